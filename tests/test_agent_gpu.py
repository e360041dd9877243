"""End-to-end parity of one agent.step(): the MI355X engine against the CPU
oracle of the reference path, on identical weights, env state, pair indices and
parameter noise (BASELINE configs[0]-like shape: few envs, T = 500)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
_DEVIATIONS = None


def _close(name, got, want, rel):
    """max |got - want| <= rel * max(1, max |want|)."""
    scale = max(1.0, want.abs().max().item())
    err = (got.double() - want.double()).abs().max().item()
    if _DEVIATIONS is not None:                 # scripts/probe_agent_tol.py
        _DEVIATIONS.append((name, err, scale))
    assert err <= rel * scale, (name, err, rel * scale)


def _forced_state(N, dof, K, td, episodes, seed):
    """Env state and parameter noise for both sides: (goal, pos0) per reset of
    a rollout -- an env resets at the start and after every episode, so
    ``episodes + 1`` of them, the last one unused -- and the noise per episode,
    all distinct.  (One episode: the draws the one-episode tests always
    made, the reset after the episode hands out the same state again.)"""
    g = torch.Generator().manual_seed(seed)
    draw_reset = lambda: (
        (torch.rand(N, dof, generator=g) * 2 - 1).to(td),
        (0.1 * (torch.rand(N, dof, generator=g) * 2 - 1)).to(td))
    draw_eps = lambda: torch.randn(N, K, generator=g).to(td)
    resets, eps = [draw_reset()], [draw_eps()]
    if episodes == 1:
        return resets * 2, eps
    resets += [draw_reset() for _ in range(episodes)]
    eps += [draw_eps() for _ in range(episodes - 1)]
    return resets, eps


def _force_resets(env, resets, td):
    """env.reset() hands out resets[0], resets[1], ... and starts over after
    the last (one rollout = one pass)."""
    N, dof = resets[0][1].shape
    turn = [0]

    def reset():
        goal, pos0 = resets[turn[0] % len(resets)]
        turn[0] += 1
        env.goal = goal.cuda()
        z = torch.zeros(N, dof, device="cuda", dtype=td)
        return env._obs(torch.zeros(N, device="cuda", dtype=td), pos0.cuda(), z)
    env.reset = reset


def _force_noise(policy, eps):
    """policy.sample() uses eps[0], eps[1], ... for its stochastic calls and
    starts over after the last (one training rollout = one pass)."""
    orig, turn = policy.sample, [0]

    def sample(**kw):
        if kw.get("use_mean"):
            return orig(**kw)
        e = eps[turn[0] % len(eps)]
        turn[0] += 1
        return orig(**kw, eps=e.cuda())
    policy.sample = sample


def build(num_env, epochs, overlap, env="metaworld", num_basis=5,
          dtype="float32", episodes=1, test_episodes=1, cfg=None, **agent_kw):
    """agent_kw: agent constructor arguments; the keys ``_contextual`` /
    ``_std_only`` switch the policy's covariance head instead.  episodes /
    test_episodes: the sampler's ``episodes_per_train_env`` /
    ``episodes_per_test_env``.  cfg: a ready experiment document (with its own
    env count, epochs and dtype) instead of tce_config's."""
    from tce_rl_amd.config import tce_config
    from tce_rl_amd.mp_exp import MPExperiment
    if cfg is None:
        cfg = tce_config(env, num_env=num_env, num_basis=num_basis,
                         epochs=epochs, evaluation_interval=0, dtype=dtype)
    cfg["params"]["sampler"]["args"].update(
        episodes_per_train_env=episodes, episodes_per_test_env=test_episodes)
    agent_kw = dict(agent_kw)
    vna = cfg["params"]["policy"]["args"]["variance_net_args"]
    if agent_kw.pop("_contextual", False):
        vna.update(contextual=True, avg_neuron=64, num_hidden=2, shape=0.0)
    if agent_kw.pop("_std_only", False):
        vna["std_only"] = True
    cfg["params"]["agent"]["args"]["overlap_updates"] = overlap
    # The reference runs its balance check in iteration 1, 26, ...
    # (num_iterations % balance_check == 1, balance_check 25 in the YAMLs);
    # those iterations take the op-by-op path.  The tests here are mostly
    # ONE iteration, so the check is off unless a case asks for it --
    # otherwise the fused / direct epochs under test would never run.
    cfg["params"]["agent"]["args"]["balance_check"] = None
    cfg["params"]["agent"]["args"].update(agent_kw)
    exp = MPExperiment()
    exp.initialize(cfg, 0, None)
    return exp.agent, cfg


class _PathSpy:
    """Counts which implementation the policy epochs went through."""

    def __init__(self, monkeypatch):
        from tce_rl_amd.rl import objective
        self.direct = self.node = 0
        run, po = objective.DirectEpoch.run, objective.policy_objective
        spy = self

        def run_spy(self_, *a, **k):
            spy.direct += 1
            return run(self_, *a, **k)

        def po_spy(*a, **k):
            spy.node += 1
            return po(*a, **k)
        monkeypatch.setattr(objective.DirectEpoch, "run", run_spy)
        monkeypatch.setattr(objective, "policy_objective", po_spy)


def to_cpu_params(net):
    return [p.detach().cpu().clone() for p in net.parameters()]


@pytest.mark.parametrize("overlap,fused,graph", [(False, True, True),
                                                 (True, True, True),
                                                 (False, False, False),
                                                 (True, False, True),
                                                 (False, True, False),
                                                 (True, True, False)])
def test_agent_step_matches_cpu_oracle(overlap, fused, graph, monkeypatch):
    """fused + graph: the objective as one autograd node, epochs replayed from a
    HIP graph; fused without graph: the epoch without autograd
    (objective.DirectEpoch); not fused: op by op."""
    spy = _PathSpy(monkeypatch)
    _agent_vs_oracle(overlap, fused, graph, "metaworld", 5)
    # the variant under test is the one that ran (3 epochs; under the graph
    # the node is called for the eager epoch and the recording)
    if fused and not graph:
        assert (spy.direct, spy.node) == (3, 0)
    elif fused:
        assert spy.direct == 0 and spy.node >= 2
    else:
        assert (spy.direct, spy.node) == (0, 0)


@pytest.mark.parametrize("env,nb,dtype,ent,iters", [
    ("metaworld", 5, "float32", 0.0, 1), ("metaworld", 5, "float32", 0.02, 3),
    ("box_push", 8, "float64", 0.0, 3), ("table_tennis", 3, "float32", 0.01, 3)])
def test_balance_check_iteration_matches_cpu_oracle(monkeypatch, env, nb,
                                                    dtype, ent, iters):
    """The reference's default: iteration 1 runs the policy balance check
    (two extra forward / backward passes per epoch,
    temporal_correlated_agent.py:447-522).  Here the objective is evaluated
    once per epoch with its gradient kept in two parts (DirectEpoch, balance):
    parameters AND both gradient norms of every epoch match the oracle, which
    runs the reference's three passes -- also with an entropy penalty, whose
    gradient belongs to neither norm, for the float64 128 x 2 box-pushing net
    and the 256 x 1 tanh table-tennis net.  iters 3 with balance_check 2: the
    iterations 1 and 3 run the check, the third with a policy that has moved
    (learning rate 1e-3: the projections are active and the trust region
    loss has a gradient worth comparing)."""
    spy = _PathSpy(monkeypatch)
    kw = dict(balance_check=2, lr_policy=1e-3) if iters > 1 else \
        dict(balance_check=25)
    agent, oracle, res = _agent_vs_oracle(
        True, True, False, env, nb, dtype, iterations=iters,
        rel_scale=1.0 if iters == 1 else 6.0, entropy_penalty_coef=ent, **kw)
    assert (spy.direct, spy.node) == (3 * iters, 0)
    sg = np.asarray(oracle.last["surrogate_grad_norm"])
    tg = np.asarray(oracle.last["trust_region_grad_norm"])
    assert len(sg) == 3 and sg.min() > 0
    print("balance norms", env, dtype, sg, tg, res["surrogate_grad_norm_mean"],
          res["trust_region_grad_norm_mean"])
    # relative to the larger of the two norms (in iteration 1 the projections
    # are inactive and the trust region gradient is rounding noise on both sides)
    rel = 1e-6 if dtype == "float64" else 2e-3
    tol = rel * max(sg.mean(), tg.mean()) * (1.0 if iters == 1 else 6.0)
    assert abs(res["surrogate_grad_norm_mean"] - sg.mean()) <= tol
    assert abs(res["trust_region_grad_norm_mean"] - tg.mean()) <= tol
    assert abs(res["surrogate_grad_norm_max"] - sg.max()) <= tol
    if iters > 1:
        assert tg.mean() > 1e-3 * sg.mean(), "the case should exercise the TR gradient"
        assert np.isclose(res["balance_ratio"], sg.mean() / tg.mean(),
                          rtol=10 * rel)


def test_balance_check_falls_back_to_op_by_op(monkeypatch):
    """Where the direct epoch does not apply (here: switched off) the balance
    check still runs, op by op, as in round 3."""
    spy = _PathSpy(monkeypatch)
    agent, oracle, res = _agent_vs_oracle(True, True, False, "metaworld", 5,
                                          balance_check=25,
                                          direct_policy_epoch=False)
    assert (spy.direct, spy.node) == (0, 0)
    sg = np.asarray(oracle.last["surrogate_grad_norm"])
    assert abs(res["surrogate_grad_norm_mean"] - sg.mean()) <= 2e-3 * sg.mean()


def test_direct_epoch_equals_autograd_epoch():
    """The policy epoch without autograd (DirectEpoch) and the same epoch
    through the autograd node: same parameters and metrics after 3 epochs."""
    out = []
    for direct in (True, False):
        torch.manual_seed(3)
        agent, _ = build(32, 3, False, direct_policy_epoch=direct,
                         graph_policy_update=False)
        torch.manual_seed(5)
        res = agent.step()
        out.append((res, [p.detach().clone()
                          for p in agent.policy.parameters]))
    (ra, pa), (rb, pb) = out
    for a, b in zip(pa, pb):
        # (two fp32 summation orders over 3 Adam steps: a few 1e-7 on weights of 1e-3 .. 1)
        torch.testing.assert_close(a, b, rtol=1e-5, atol=5e-7)
    for k in ("surrogate_loss_mean", "trust_region_loss_mean", "entropy_mean",
              "policy_grad_norm_mean", "projection_new_old_cov_diff_mean",
              "projection_proj_old_mean_diff_mean"):
        assert abs(ra[k] - rb[k]) <= 1e-5 * abs(rb[k]) + 1e-7, k


@pytest.mark.parametrize("env,nb,dtype", [
    ("metaworld", 8, "float32"), ("box_push", 8, "float32"),
    ("box_push", 3, "float32"), ("table_tennis", 3, "float32"),
    ("table_tennis", 8, "float32"),
    ("box_push", 3, "float64"), ("metaworld", 5, "float64")])
def test_agent_step_matches_cpu_oracle_other_shapes(env, nb, dtype):
    """K 36 (the reference's Metaworld basis count) and the 7-dof box-pushing
    shapes (K 63 / 28, T 100, 256-wide leaky-relu critic on the library path);
    table tennis: T 350, phase delay 0.3, tanh policy, MDP-reward re-shaping
    -- with the reference's 3 basis functions (K 28) and with the 8 that
    BASELINE.json configs[4] states (K 63)."""
    _agent_vs_oracle(True, True, False, env, nb, dtype)


def test_agent_step_matches_cpu_oracle_hopper_document():
    """The one shipped document whose shape no other oracle comparison has:
    tests/golden/resolved/hopper_jump_tcp.json -- float64, dof 3, 3 basis
    functions (K 12: run-time-shape trajectory rows kernel with 8-byte chunks,
    LDS form of the pair kernels at R 6), T 250, has_left_floor reward
    re-shaping -- shrunk to 6 envs x 2 episodes and 3 + 3 epochs, two
    iterations, at the float64 tolerances of the other cases."""
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    d = json.load(open(os.path.join(here, "golden", "resolved",
                                    "hopper_jump_tcp.json")))
    p, N, EPOCHS = d["params"], 6, 3
    assert p["mp"]["args"]["num_dof"] == 3 and \
        p["mp"]["args"]["num_basis"] == 3 and \
        p["agent"]["args"]["dtype"] == "float64"
    for blk in p.values():
        blk["args"]["device"] = "cuda"
    p["sampler"]["args"].update(num_env_train=N, num_env_test=N,
                                task_specified_metrics=["success"])
    p["agent"]["args"].update(epochs_policy=EPOCHS, epochs_critic=EPOCHS,
                              evaluation_interval=0)
    p["policy"]["args"]["mp"] = p["mp"]
    cfg = {"name": d["name"], "seed": 0, "iterations": d["iterations"],
           "params": p}
    agent, oracle, _ = _agent_vs_oracle(
        True, True, False, "hopper", 3, "float64", iterations=2, num_env=N,
        epochs=EPOCHS, episodes=2, cfg=cfg)
    assert agent.sampler.num_times == oracle.T == 250
    assert agent.policy.num_dof == 3 and agent.policy.dim_out == 12


@pytest.mark.parametrize("overlap", [False, True])
def test_agent_step_matches_cpu_oracle_split_f16_critic(overlap):
    """critic_arith="f16x2" (split-f16 matrix-core critic epochs) is held to
    the same tolerances against the CPU oracle as the exact-fp32 kernel."""
    _agent_vs_oracle(overlap, True, False, "metaworld", 5, critic_arith="f16x2")


@pytest.mark.parametrize("overlap", [False, True])
def test_agent_step_matches_cpu_oracle_bf16x3_critic(overlap):
    """critic_arith="bf16x3" (three-part bf16 operands: 24 bits, fp32's range)
    is held to the same tolerances against the CPU oracle as the exact-fp32
    kernel."""
    _agent_vs_oracle(overlap, True, False, "metaworld", 5, critic_arith="bf16x3")


def _agent_vs_oracle(overlap, fused, graph, env, nb, dtype="float32",
                     iterations=1, rel_scale=1.0, num_env=16, epochs=3,
                     episodes=1, critic_vs_oracle=True, **kw):
    """episodes: per env and rollout, each from its own forced reset with its
    own noise -- the dataset has ``num_env * episodes`` rows.
    critic_vs_oracle False: the critic's minibatches are not the oracle's
    (device-drawn permutations), its parameters are not compared."""
    from oracle.agent_oracle import OracleTCE
    N, EPOCHS = num_env, epochs
    agent, cfg = build(N, EPOCHS, overlap, env=env, num_basis=nb, dtype=dtype,
                       fused_policy_objective=fused,
                       graph_policy_update=graph, episodes=episodes, **kw)
    oracle = OracleTCE(cfg["params"], N, total_iterations=cfg["iterations"],
                       episodes=episodes)
    # identical weights
    with torch.no_grad():
        for po, pg in zip(oracle.pnet, agent.policy.mean_net.parameters()):
            po.copy_(pg.cpu())
        for po, pg in zip(oracle.cnet, agent.critic.net.parameters()):
            po.copy_(pg.cpu())
        for po, pg in zip(oracle.var_params,
                          agent.policy.variance_net.parameters()):
            po.copy_(pg.cpu())
    # identical env state and noise
    td = torch.float64 if dtype == "float64" else torch.float32
    resets, eps = _forced_state(N, agent.policy.num_dof, agent.policy.dim_out,
                                td, episodes, 7)
    _force_resets(agent.sampler.train_envs, resets, td)
    _force_noise(agent.policy, eps)
    oracle.forced_reset, oracle.forced_eps = resets, eps

    captured = {}
    orig_pd = agent.process_dataset

    def pd(ds):
        out = orig_pd(ds)
        captured.update({k: v.detach().cpu() for k, v in out.items()
                         if torch.is_tensor(v) and k != "segment_params_L"})
        return out
    agent.process_dataset = pd

    # pair offset (torch's global CPU generator) and minibatch permutations
    # (numpy's, util_data_structure.py:389-390): same host draws on both sides
    torch.manual_seed(11)
    np.random.seed(13)
    for _ in range(iterations):
        res = agent.step()
    torch.manual_seed(11)
    np.random.seed(13)
    for _ in range(iterations):
        oracle.step()
    ref = oracle.last
    assert np.array_equal(agent.sampler.pred_pairs.cpu().numpy(),
                          ref["pred_pairs"].numpy())           # bit-exact indexing
    # Tolerances: max |gpu - oracle| <= rel * max(1, max |oracle|) per tensor,
    # rel = 8-10 x the largest deviation seen over every case of this file
    # (scripts/probe_agent_tol.py, table in DESIGN.md section 5) -- all of it
    # float32 rounding, nothing structural:
    #  * actions: a K-term dot product of basis values and parameters, a few
    #    eps32 = 6e-8 per term (seen 2e-7 relative);
    #  * values: three 128-wide layers (2e-6); returns / advantages: the
    #    lambda-discounted scan over T steps adds the value errors of the later
    #    steps, relative to max |return| that is still 3e-7;
    #  * log-prob: north_star's 1e-5.  The pair covariance has a 1e-4 floor;
    #    the kernels form and factor it in double (round 6) and sit <= 1e-6
    #    of max |logp| from the float64 value (tests/test_prodmp_gpu.py), so
    #    what is seen here (3.7e-6) is the float32 ORACLE's own distance from
    #    it -- the reference's float32 arithmetic has the same;
    #  * parameters after EPOCHS Adam steps: Adam's step lr m / (sqrt v + eps)
    #    is scale free, so a relative gradient error delta moves a parameter by
    #    ~ lr * delta per step; the policy's gradient passes the projection's
    #    implicit derivative (seen 5e-5 of max |w|), the critic's 8e-6.
    # float64 runs: the rollout quantities keep a floor of ~1e-6: the product's
    # and the oracle's ProDMP tables are ONE derivation written twice (numpy
    # there, torch here), so this floor is the difference between the two
    # libraries evaluating the same closed forms -- what bounds both tables is
    # the independent ODE integration of tests/test_prodmp_ode_cpu.py; the
    # parameters agree to 1e-7.
    f64 = dtype == "float64"

    close = lambda name, got, want, rel: _close(name, got, want,
                                                rel * rel_scale)
    close("step_actions", captured["step_actions"], ref["step_actions"], 3e-6)
    close("step_rewards", captured["step_rewards"], ref["step_rewards"], 3e-6)
    close("step_values", captured["step_values"], ref["step_values"], 2e-5)
    close("step_returns", captured["step_returns"], ref["step_returns"], 5e-6)
    close("step_advantages", captured["step_advantages"],
          ref["step_advantages"], 5e-6)
    close("segment_advantage", captured["segment_advantage"],
          ref["segment_advantage"], 5e-6)
    # (north_star's bound as it stands, also after a second iteration)
    _close("segment_log_prob_estimate", captured["segment_log_prob_estimate"],
           ref["segment_log_prob_estimate"], 1e-5)
    # parameters after EPOCHS critic + policy updates
    for pg, po in zip(agent.critic.net.parameters(), oracle.cnet):
        if critic_vs_oracle:
            close("critic", pg.detach().cpu(), po.detach(),
                  1e-7 if f64 else 5e-5)
    for pg, po in zip(agent.policy.mean_net.parameters(), oracle.pnet):
        close("policy", pg.detach().cpu(), po.detach(), 1e-6 if f64 else 3e-4)
    for pg, po in zip(agent.policy.variance_net.parameters(),
                      oracle.var_params):
        close("variance", pg.detach().cpu(), po.detach(),
              1e-6 if f64 else 3e-5)
    assert np.isfinite(res["critic_loss_mean"])
    if episodes > 1:
        _check_episode_rows(agent, oracle, captured, N, episodes)
    return agent, oracle, res


def _check_episode_rows(agent, oracle, captured, N, episodes):
    """What only shows with several episodes: the dataset has N * episodes
    rows, every episode was normalised with the observation statistics of ITS
    moment, and the statistics have seen every row once (tolerances: those of
    tests/test_rollout_gpu.py for the statistics and the normalised rows)."""
    ref, rms = oracle.last, agent.sampler.obs_rms
    T = agent.sampler.num_times
    R = N * episodes
    assert captured["step_actions"].shape[0] == R
    assert captured["step_states"].shape[:2] == (R, T)
    # statistics: float32 at tests/test_rollout_gpu.py's 2e-5 (seen here:
    # 1.4e-7, table tennis variance).  float64: THERE the kernel gets the
    # oracle's very rows and the bound is 1e-10; HERE the rows come from each
    # side's own ProDMP table, which agree to ~1e-6 (see _agent_vs_oracle:
    # step_actions seen 2.2e-7 in this float64 case), so the statistics cannot
    # agree to 1e-10 -- seen 9.5e-10 (variance, after four merges), bound 1e-8
    f64 = ref["step_states"].dtype == torch.float64
    tol = 1e-8 if f64 else 2e-5
    _close("obs_rms_mean", rms.mean.cpu(), ref["obs_rms_mean"], tol)
    _close("obs_rms_var", rms.var.cpu(), ref["obs_rms_var"], tol)
    assert abs(rms.count - ref["obs_rms_count"]) < 1e-6
    assert rms.count == pytest.approx(
        1e-4 + agent.num_iterations * R * (T + 1), rel=1e-12)
    # normalised rows at test_rollout_gpu.py's 1e-5 (seen: 3.5e-6 float32,
    # 6.3e-7 float64 -- the actions' deviation divided by the columns' std)
    stol = 1e-5
    _close("step_states", captured["step_states"], ref["step_states"][:, :-1],
           stol)
    # the first episode's rows under the FINAL statistics are something else:
    # the comparison above does tell "per episode" from "once at the end"
    first = ref["segment_state"][:N]
    with_final = (first - ref["obs_rms_mean"]) / torch.sqrt(
        ref["obs_rms_var"] + 1e-8)
    assert (ref["step_states"][:N, 0] - with_final).abs().max() > 100 * stol


EPISODE_CASES = {
    # the statistics carried over two iterations (four merges), float64
    "box_push_f64_2x2": dict(env="box_push", nb=3, dtype="float64", num_env=12,
                             episodes=2, iterations=2),
    # MDP reward with each episode's own hit_ball flags; 33 rows
    "table_tennis_3": dict(env="table_tennis", nb=3, num_env=11, episodes=3),
    # 22 rows x 500 steps in 4 minibatches of numpy's permutation
    "metaworld_minibatches": dict(env="metaworld", nb=5, num_env=11,
                                  episodes=2, num_minibatchs=4),
    # per-row Cholesky factors: the concatenation materialises [N * E, K, K]
    "metaworld_contextual": dict(env="metaworld", nb=5, num_env=11, episodes=2,
                                 _contextual=True),
}


@pytest.mark.parametrize("case", sorted(EPISODE_CASES))
def test_agent_step_of_several_episodes_matches_cpu_oracle(case, monkeypatch):
    """agent.step() with ``episodes_per_train_env`` > 1 against the CPU oracle
    running the same episodes: every episode from its own reset with its own
    noise, ONE pair draw, observation statistics updated and applied episode
    by episode, rows concatenated episode-major -- and N * E rows (a number
    the kernels do not tile by) through GAE, the segment advantage, the critic
    and the policy epochs.  Tolerances: the one-episode table, x 2 for a second
    iteration."""
    kw = dict(EPISODE_CASES[case])
    env, nb = kw.pop("env"), kw.pop("nb")
    iters = kw.get("iterations", 1)
    spy = _PathSpy(monkeypatch)
    agent, oracle, res = _agent_vs_oracle(
        True, True, False, env, nb, epochs=2, rel_scale=float(iters), **kw)
    if kw.get("_contextual"):
        assert agent.last_policy_plan.kind == "op_by_op"
    if "num_minibatchs" in kw:
        assert tuple(agent.last_critic_plan)[:2] == ("fused-narrow", 4)
        assert (spy.direct, spy.node) == (2 * iters, 0)


def test_agent_step_of_several_episodes_with_device_drawn_minibatches():
    """The same with ``minibatch_permutation: device`` (a keyed permutation of
    the N * E * T rows drawn on the device): the pieces are not the oracle's, so
    the rollout, the advantages and the policy -- which does not see this
    iteration's critic update -- are compared with it, and the critic is held
    to what tests/test_minibatch_gpu.py holds it to: the fused minibatch
    epochs ran, and the same seeds give the same parameters bit for bit."""
    out = []
    for _ in range(2):
        agent, _, _ = _agent_vs_oracle(
            True, True, False, "metaworld", 5, num_env=11, epochs=2,
            episodes=2, num_minibatchs=4, minibatch_permutation="device",
            critic_vs_oracle=False)
        assert tuple(agent.last_critic_plan)[:2] == ("fused-narrow", 4)
        out.append(torch.cat([p.detach().reshape(-1)
                              for p in agent.critic.parameters]).clone())
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("env,nb,dtype,N,iters", [
    ("metaworld", 5, "float32", 4096, 2), ("box_push", 8, "float64", 2048, 1)])
def test_large_batch_step_matches_cpu_oracle(env, nb, dtype, N, iters,
                                             monkeypatch):
    """The oracle comparison at sizes where the large-grid code paths run
    (every other oracle case is 16 - 24 envs): BASELINE
    configs[1] at its full 4096 envs x T 500 -- 2 M critic rows on the
    224-workgroup persistent grid with several tiles per workgroup, per-workgroup
    gradient slabs, 64-env blocks of the pair kernels, the adaptive critic split
    taken from the first iteration's events in the second -- and the box-pushing
    shape in float64 at 2048 envs (205 k rows on the two-launch wide critic, the
    float64 128 x 2 policy net on csrc/pmlp.hip with 64 row tiles), 2 + 2 epochs,
    overlapped updates.  Same tolerances as the small cases (x 2 for the second
    iteration)."""
    spy = _PathSpy(monkeypatch)
    agent, oracle, res = _agent_vs_oracle(
        True, True, False, env, nb, dtype, iterations=iters, num_env=N, epochs=2,
        rel_scale=float(iters))
    assert (spy.direct, spy.node) == (2 * iters, 0)
    if iters > 1:
        assert 0 < agent._critic_split <= 2 or agent._critic_split == 0


@pytest.mark.parametrize("env,nb", [("metaworld", 5), ("table_tennis", 3)])
def test_deterministic_evaluation_matches_cpu_oracle(env, nb):
    _evaluation_vs_oracle(env, nb)


def test_deterministic_evaluation_of_two_episodes_matches_cpu_oracle():
    _evaluation_vs_oracle("table_tennis", 3, test_episodes=2)


def _evaluation_vs_oracle(env, nb, test_episodes=1):
    """f4: AbstractAgent.evaluate (abstract_agent.py:219-255) =
    one deterministic test rollout (use_mean, temporal_correlated_sampler.py:
    305-315): the trajectory of the mean parameters, raw (un-normalised) states
    into the critic, observation statistics untouched, pair offsets drawn --
    after one training step, against the CPU oracle's evaluate().
    test_episodes 2: ``episodes_per_test_env``, every episode from its own
    reset, rows concatenated over the episodes."""
    from oracle.agent_oracle import OracleTCE
    N = 16
    agent, cfg = build(N, 2, True, env=env, num_basis=nb,
                       test_episodes=test_episodes)
    oracle = OracleTCE(cfg["params"], N, test_episodes=test_episodes)
    with torch.no_grad():
        for po, pg in zip(oracle.pnet, agent.policy.mean_net.parameters()):
            po.copy_(pg.cpu())
        for po, pg in zip(oracle.cnet, agent.critic.net.parameters()):
            po.copy_(pg.cpu())
        oracle.var.copy_(agent.policy.variance_net.variable.cpu())
    # (the training rollout: one episode from the first reset; the evaluation:
    # test_episodes episodes from the first resets of the same list)
    resets, eps = _forced_state(N, agent.policy.num_dof, agent.policy.dim_out,
                                torch.float32, test_episodes, 9)
    _force_resets(agent.sampler.train_envs, [resets[0]], torch.float32)
    _force_resets(agent.sampler.test_envs, resets, torch.float32)
    _force_noise(agent.policy, eps[:1])
    oracle.forced_reset, oracle.forced_eps = resets, eps[0]
    torch.manual_seed(11)
    agent.step()
    torch.manual_seed(11)
    oracle.step()
    rms_before = (agent.sampler.obs_rms.mean.clone(),
                  agent.sampler.obs_rms.var.clone(), agent.sampler.obs_rms.count)
    torch.manual_seed(12)
    det, sto = agent.evaluate()
    torch.manual_seed(12)
    ref = oracle.evaluate()
    assert sto == {}
    assert np.array_equal(agent.sampler.pred_pairs.cpu().numpy(),
                          ref["pred_pairs"].numpy())
    # the policy / critic differ by one fp32 training step (parameters agree to
    # 3e-4 there, see _agent_vs_oracle); the evaluation rollout itself adds
    # float32 rounding only.  Bounds = 10 x the largest deviation seen
    # (scripts/probe_agent_tol.py).
    c = lambda k: det[k].detach().cpu()
    _close("eval step_actions", c("step_actions"), ref["step_actions"], 1e-5)
    _close("eval step_rewards", c("step_rewards"), ref["step_rewards"], 1e-5)
    _close("eval episode_reward", c("episode_reward"), ref["episode_reward"],
           3e-6)
    _close("eval step_values", c("step_values"), ref["step_values"], 1e-5)
    _close("eval log_prob", c("segment_log_prob_estimate"),
           ref["segment_log_prob_estimate"], 1e-5)
    assert torch.equal(c("success"), ref["success"])
    assert c("step_actions").shape[0] == N * test_episodes
    if test_episodes > 1:       # the episodes are not copies of each other
        assert not torch.allclose(c("step_actions")[:N], c("step_actions")[N:])
    # deterministic: the trajectory is the one of the mean parameters
    mean = det["segment_params_mean"]
    from tce_rl_amd import ops
    t0 = det["segment_init_time"]
    again = ops.prodmp_traj(agent.policy.mp,
                            agent.sampler.get_times(t0, agent.sampler.num_times),
                            mean, t0, det["segment_init_pos"],
                            det["segment_init_vel"])
    torch.testing.assert_close(det["step_actions"], again)
    # raw states went to the critic and the statistics did not move
    s = det["step_states_full"]
    assert torch.equal(s[:, 0], det["segment_state"])
    assert torch.equal(agent.sampler.obs_rms.mean, rms_before[0])
    assert torch.equal(agent.sampler.obs_rms.var, rms_before[1])
    assert agent.sampler.obs_rms.count == rms_before[2]


def test_checkpoint_round_trip(tmp_path):
    """save_agent / load_agent (reference file naming and formats)."""
    agent, _ = build(8, 1, False)
    agent.step()
    agent.save_agent(str(tmp_path), 1)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert "ValueFunction_mlp_parameters.pkl" in names
    assert "ValueFunction_mlp_weights_1" in names
    assert "TemporalCorrelatedPolicy_mean_mlp_weights_1" in names
    assert "TemporalCorrelatedPolicy_variance_variable_weights_1" in names
    assert "policy_optimizer_state_1" in names and "obs_rms_state_1" in names
    before = [p.detach().clone() for p in agent.policy.parameters]
    agent2, _ = build(8, 1, False)
    agent2.load_agent(str(tmp_path), 1)
    for a, b in zip(before, agent2.policy.parameters):
        assert torch.equal(a, b.detach())
    assert agent2.num_iterations == 1
    torch.testing.assert_close(agent2.sampler.obs_rms.mean,
                               agent.sampler.obs_rms.mean)


@pytest.mark.parametrize("env", ["box_push", "table_tennis"])
def test_other_tce_configs_step(env):
    """BASELINE configs[2] / [4] shapes at reduced env count: dof 7, K 63 / 28,
    leaky_relu / tanh nets (library-GEMM critic path), MDP reward re-shaping."""
    from tce_rl_amd.config import tce_config
    from tce_rl_amd.mp_exp import MPExperiment
    nb = 8 if env == "box_push" else 3
    cfg = tce_config(env, num_env=96, num_basis=nb, epochs=2,
                     evaluation_interval=1, num_env_test=16)
    exp = MPExperiment()
    exp.initialize(cfg, 0, None)
    for i in range(2):
        res = exp.iterate(cfg, 0, i)
    for k in ("critic_loss_mean", "surrogate_loss_mean", "entropy_mean",
              "projection_proj_old_cov_diff_mean",
              "evaluation_episode_reward_mean"):
        assert np.isfinite(res[k]), k
    assert res["projection_proj_old_cov_diff_mean"] <= \
        cfg["params"]["projection"]["args"]["cov_bound"] * 1.01


BB_MP = dict(num_dof=4, num_basis=4, tau=5.0, alpha_phase=3, alpha=10,
             dt=0.0125, basis_bandwidth_factor=5, weights_scale=0.1,
             goal_scale=0.1, relative_goal=True)


def build_bbrl(num_env, epochs, policy_hidden=(32, 2), critic_hidden=(32, 2),
               act="relu", std_only=True, dtype="float32", episodes=1,
               **agent_kw):
    """policy_hidden / critic_hidden: (neurons, hidden layers); episodes: the
    sampler's ``episodes_per_train_env``."""
    from tce_rl_amd.rl import (agent_factory, critic_factory, policy_factory,
                               projection_factory, sampler_factory)
    mp = {"type": "prodmp", "args": dict(BB_MP, dtype=dtype, device="cuda")}
    sampler = sampler_factory("BlackBoxSampler",
                              env_id="metaworld_ProDMP/push-v2",
                              num_env_train=num_env, num_env_test=16,
                              episodes_per_train_env=episodes,
                              dtype=dtype, device="cuda", seed=0, mp=mp,
                              task_specified_metrics=["success"])
    d_in = sampler.observation_shape[-1]
    common = dict(init_method="orthogonal", act_func_hidden=act,
                  act_func_last=None, dtype=dtype, device="cuda")
    policy = policy_factory(
        "BlackBoxPolicy", dim_in=d_in, dim_out=20,
        mean_net_args=dict(avg_neuron=policy_hidden[0],
                           num_hidden=policy_hidden[1], shape=0.0),
        variance_net_args=dict(std_only=std_only, contextual=False),
        out_layer_gain=0.01, min_std=1e-5, **common)
    critic = critic_factory("ValueFunction", dim_in=d_in, dim_out=1,
                            hidden=dict(avg_neuron=critic_hidden[0],
                                        num_hidden=critic_hidden[1], shape=0.0),
                            out_layer_gain=1, **common)
    proj = projection_factory(
        "KLProjectionLayer", proj_type="kl", mean_bound=0.005,
        cov_bound=0.0005, trust_region_coeff=1.0, entropy_schedule=False,
        action_dim=20, total_train_steps=100, dtype=dtype, device="cuda")
    kw = dict(lr_policy=3e-4, lr_critic=3e-4, wd_policy=0.0,
              wd_critic=0.0, discount_factor=1, epochs_policy=epochs,
              epochs_critic=epochs, num_minibatchs=1, norm_advantages=True,
              clip_advantages=0.0, set_variance=True, balance_check=25,
              evaluation_interval=1, dtype=dtype, device="cuda")
    kw.update(agent_kw)
    agent = agent_factory(
        "BlackBoxAgent", policy=policy, critic=critic, sampler=sampler,
        projection=proj, **kw)
    return agent, d_in


def test_bbrl_agent_step():
    """BASELINE configs[3]-like: black-box agent, diagonal covariance, K 20."""
    agent, _ = build_bbrl(256, 3)
    for _ in range(2):
        res = agent.step()
    assert np.isfinite(res["critic_loss_mean"])
    assert np.isfinite(res["projection_kl"])
    assert res["num_global_steps"] == 2 * 256 * 500


def test_bbrl_graph_epochs_equal_eager_epochs():
    """BlackBoxAgent: epochs replayed from HIP graphs (default) == the same
    epochs launched eagerly (5 epochs: one eager, one captured, four replays)."""
    out = []
    for graph in (True, False):
        torch.manual_seed(0)
        agent, _ = build_bbrl(64, 5)
        agent.small_net_kernels = False         # the op-by-op epochs
        agent.graph_epochs = graph
        agent.evaluation_interval = 0
        torch.manual_seed(1)
        res = agent.step()
        out.append((res, [p.detach().clone() for p in
                          agent.policy.parameters + agent.critic.parameters]))
    (ra, pa), (rb, pb) = out
    for a, b in zip(pa, pb):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-8)
    for k in ("critic_loss_mean", "surrogate_loss_mean", "policy_grad_norm_mean",
              "projection_kl", "entropy_mean"):
        assert abs(ra[k] - rb[k]) <= 1e-6 * abs(rb[k]) + 1e-8, k


def test_bbrl_kept_graphs_equal_fresh_graphs_over_iterations():
    """The black-box agent keeps the HIP graphs of its two updates across
    iterations (inputs copied into static buffers, the two graphs replayed on
    two streams).  Three iterations -- new rollouts, so new inputs -- end with
    the parameters of an agent that records its epochs anew every time, and of
    one that launches them eagerly one update after the other."""
    out = []
    for kw in (dict(), dict(cache_epoch_graphs=False),
               dict(graph_epochs=False, overlap_updates=False)):
        torch.manual_seed(0)
        agent, _ = build_bbrl(96, 6)
        agent.small_net_kernels = False         # the op-by-op epochs
        for k, v in kw.items():
            setattr(agent, k, v)
        agent.evaluation_interval = 0
        torch.manual_seed(1)
        for _ in range(3):
            res = agent.step()
        out.append((res, [p.detach().clone() for p in
                          agent.policy.parameters + agent.critic.parameters],
                    agent.policy_optimizer.host_step,
                    float(agent.policy_optimizer.dev_state[0])))
    assert agent.num_global_steps == out[0][0]["num_global_steps"]
    for res, params, host_step, dev_step in out:
        assert host_step == dev_step == 18          # 3 iterations x 6 epochs
        for a, b in zip(params, out[2][1]):
            torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-8)
        for k in ("critic_loss_mean", "surrogate_loss_mean", "entropy_mean"):
            assert abs(res[k] - out[2][0][k]) <= 1e-6 * abs(out[2][0][k]) + 1e-8


@pytest.mark.parametrize("mode", ["small", "op_by_op", "fused",
                                  "small_minibatch3"])
def test_bbrl_step_matches_cpu_oracle(mode, monkeypatch):
    _bbrl_step_vs_oracle(mode, monkeypatch)


@pytest.mark.parametrize("mode", ["small", "small_minibatch3"])
def test_bbrl_step_matches_cpu_oracle_two_episodes(mode, monkeypatch):
    _bbrl_step_vs_oracle(mode, monkeypatch, episodes=2)


def _bbrl_step_vs_oracle(mode, monkeypatch, episodes=1):
    """One BlackBoxAgent.step() (a16) against the CPU oracle step on the same
    weights, env state and parameter noise: on the hand-written row kernels of
    csrc/smlp.hip (the default), op by op under autograd, and with the
    objective as one autograd node.  episodes 2: two episodes per env, each
    from its own reset with its own noise (black_box_sampler.py:158-249) --
    N * 2 = 22 rows, not a multiple of what the row kernels tile by."""
    from oracle.agent_oracle import OracleBBRL
    from tce_rl_amd import smlp_ops
    N, EPOCHS = (24, 3) if episodes == 1 else (11, 3)
    agent, d_in = build_bbrl(N, EPOCHS, episodes=episodes)
    agent.evaluation_interval = 0
    # small_minibatch3: the critic's minibatches (black_box_agent.py:124-131;
    # the class default is 10) on the row kernels, gathered pieces of numpy's
    # permutation -- same path assertions as "small"
    nmb = 3 if mode == "small_minibatch3" else 1
    mode = "small" if nmb > 1 else mode
    agent.num_minibatchs = nmb
    agent.small_net_kernels = mode == "small"
    agent.fused_policy_objective = mode == "fused"   # tce_bb_policy_objective_*
    calls = {"c": 0, "p": 0}
    cu, pu = smlp_ops.critic_update, smlp_ops.policy_update
    monkeypatch.setattr(smlp_ops, "critic_update", lambda *a, **k: (
        calls.__setitem__("c", calls["c"] + 1), cu(*a, **k))[1])
    monkeypatch.setattr(smlp_ops, "policy_update", lambda *a, **k: (
        calls.__setitem__("p", calls["p"] + 1), pu(*a, **k))[1])
    # (iteration 1 = 1 mod balance_check: the row-kernel path runs the balance
    # check, black_box_agent.py:218-284; the other two paths do not have it)
    oracle = OracleBBRL(BB_MP, N, d_in, [32, 32], [32, 32], "relu", True, 1e-5,
                        0.01, 3e-4, EPOCHS, 0.005, 0.0005, 1.0, True,
                        balance=mode == "small", num_minibatchs=nmb,
                        episodes=episodes)
    with torch.no_grad():
        for po, pg in zip(oracle.pnet, agent.policy.mean_net.parameters()):
            po.copy_(pg.cpu())
        for po, pg in zip(oracle.cnet, agent.critic.net.parameters()):
            po.copy_(pg.cpu())
        oracle.var.copy_(agent.policy.variance_net.variable.cpu())
    resets, eps = _forced_state(N, 4, 20, torch.float32, episodes, 3)
    _force_resets(agent.sampler.train_envs, resets, torch.float32)
    _force_noise(agent.policy, eps)
    oracle.forced_reset, oracle.forced_eps = resets, eps
    captured = {}
    pd = agent.process_dataset

    def grab(ds):
        out = pd(ds)
        captured.update({k: v.detach().cpu() for k, v in out.items()
                         if torch.is_tensor(v) and k != "segment_params_L"})
        return out
    agent.process_dataset = grab
    np.random.seed(5)                       # (the minibatch permutations)
    res = dict(agent.step())
    np.random.seed(5)
    oracle.step()
    ref = oracle.last
    assert captured["segment_action"].shape[0] == N * episodes
    _check_bbrl_metrics(res, oracle, 2e-4, balance=mode == "small")
    # float32 rounding only: bounds = 10-30 x the largest deviation seen
    # (32-wide nets, diagonal covariance: shorter sums than the TCE step)
    _close("segment_action", captured["segment_action"], ref["segment_action"],
           3e-6)
    _close("segment_log_prob", captured["segment_log_prob"],
           ref["segment_log_prob"], 2e-6)
    _close("segment_value", captured["segment_value"], ref["segment_value"],
           2e-6)
    _close("segment_reward", captured["segment_reward"], ref["segment_reward"],
           2e-6)
    _close("segment_advantage", captured["segment_advantage"],
           ref["segment_advantage"], 5e-6)
    for pg, po in zip(agent.critic.net.parameters(), oracle.cnet):
        _close("critic", pg.detach().cpu(), po.detach(), 2e-6)
    for pg, po in zip(agent.policy.mean_net.parameters(), oracle.pnet):
        _close("policy", pg.detach().cpu(), po.detach(), 3e-6)
    _close("variance", agent.policy.variance_net.variable.detach().cpu(),
           oracle.var.detach(), 3e-6)
    assert (calls["c"], calls["p"]) == ((1, 1) if mode == "small" else (0, 0))


_KL_KEYS = ["projection_%s_%s" % (a, b)
            for a in ("new_old", "new_proj", "proj_old")
            for b in ("mean_diff", "cov_diff", "shape_diff", "volume_diff")]


def _check_bbrl_metrics(res, oracle, f32_rel, balance):
    """The reference's per-epoch diagnostics of the black-box policy update
    (black_box_agent.py:345-375): the 12 KL means of kl_old_new_proj and --
    balance-check iterations -- the two gradient norms, against the oracle's."""
    want = np.array(oracle.kl_rows)
    assert want.shape[1] == 12
    # (the cov / shape / volume parts are differences of O(K) terms -- trace - K,
    # log-determinants: in float32 they carry ~K eps of absolute error on both
    # sides, the oracle's included)
    tol = f32_rel * max(np.abs(want).max(), 1e-12) + (1e-5 if f32_rel > 1e-6
                                                       else 1e-12)
    for i, k in enumerate(_KL_KEYS):
        assert abs(res[k + "_mean"] - want[:, i].mean()) <= tol, \
            (k, res[k + "_mean"], want[:, i].mean())
        assert abs(res[k + "_max"] - want[:, i].max()) <= tol, k
    if balance:
        bn = np.array(oracle.balance_norms)
        assert bn.shape == (len(want), 2)
        assert res["surrogate_grad_norm_mean"] == pytest.approx(
            bn[:, 0].mean(), rel=10 * f32_rel)
        assert res["trust_region_grad_norm_mean"] == pytest.approx(
            bn[:, 1].mean(), rel=10 * f32_rel, abs=1e-7)
        if bn[:, 1].mean() > 0:
            assert res["balance_ratio"] == pytest.approx(
                bn[:, 0].mean() / bn[:, 1].mean(), rel=20 * f32_rel)
    else:
        assert "balance_ratio" not in res


BBRL_MID = {
    # mprl/config/box_push_random_init/bbrl/entire/shared.yaml:4,66-67,84-85,31-33
    "box_push": dict(policy_hidden=(128, 2), critic_hidden=(256, 2),
                     act="leaky_relu", std_only=False, dtype="float32",
                     wd=5e-5, clip_critic=0.0),
    # mprl/config/table_tennis_4d/bbrl/entire/shared.yaml:72-73,90-91,31-33
    "table_tennis": dict(policy_hidden=(256, 1), critic_hidden=(256, 1),
                         act="leaky_relu", std_only=False, dtype="float32",
                         wd=1e-5, clip_critic=0.0),
    # the same row kernels in float64, a tanh net, a clipped value loss
    "f64_clip": dict(policy_hidden=(128, 2), critic_hidden=(128, 2),
                     act="tanh", std_only=False, dtype="float64", wd=0.0,
                     clip_critic=0.2),
    "f64_one_layer": dict(policy_hidden=(128, 1), critic_hidden=(128, 1),
                          act="relu", std_only=True, dtype="float64", wd=0.0,
                          clip_critic=0.2),
}


@pytest.mark.parametrize("balance,nmb", [(False, 1), (True, 1), (False, 4)])
@pytest.mark.parametrize("shape", sorted(BBRL_MID))
def test_bbrl_midsize_nets_match_cpu_oracle(shape, balance, nmb, monkeypatch):
    _bbrl_midsize_vs_oracle(shape, balance, nmb, monkeypatch)


@pytest.mark.parametrize("shape,nmb", [("box_push", 1), ("table_tennis", 4)])
def test_bbrl_midsize_nets_match_cpu_oracle_two_episodes(shape, nmb,
                                                         monkeypatch):
    """The same with two episodes per env, each from its own reset with its own
    noise: 11 x 2 = 22 rows through the matrix-core critic epochs / the row
    kernels and the one-call policy epochs, at the one-episode tolerances.
    (float32 shapes only: the float64 shapes' 1e-10 bound on the episode
    return holds for the 24 env states of the one-episode cases, other states
    -- 11 envs, ONE episode -- reach 4e-9 of max |return| in single rows.)"""
    _bbrl_midsize_vs_oracle(shape, False, nmb, monkeypatch, num_env=11,
                            episodes=2)


def _bbrl_midsize_vs_oracle(shape, balance, nmb, monkeypatch, num_env=24,
                            episodes=1):
    """One BlackBoxAgent.step() with the reference's OTHER black-box nets -- box
    pushing's 128 x 2 policy / 256 x 2 critic, table tennis's 256 x 1 / 256 x 1
    (full covariance, leaky relu, weight decay) -- against the CPU oracle: the
    policy epochs as ONE C call each (objective.BBDirectEpoch), the critic on
    the matrix-core epochs (256 x 2) or the row kernels of csrc/pmlp.hip; no
    autograd, no library GEMM.  balance: an iteration with the policy balance
    check (black_box_agent.py:218-284), its two gradient norms included."""
    from oracle.agent_oracle import OracleBBRL
    from tce_rl_amd import mlp_ops, pmlp_ops
    from tce_rl_amd.rl import objective
    cfg = BBRL_MID[shape]
    # (balance: more and larger steps, so that the trust region becomes active
    # and its loss has a gradient to measure)
    N, EPOCHS, LR = (num_env, 6, 3e-3) if balance else (num_env, 3, 3e-4)
    dt = getattr(torch, cfg["dtype"])
    agent, d_in = build_bbrl(
        N, EPOCHS, cfg["policy_hidden"], cfg["critic_hidden"], cfg["act"],
        cfg["std_only"], cfg["dtype"], episodes=episodes,
        wd_policy=cfg["wd"], wd_critic=cfg["wd"],
        clip_critic=cfg["clip_critic"], balance_check=25 if balance else False,
        lr_policy=LR, lr_critic=LR)
    agent.evaluation_interval = 0
    # nmb 4: the critic's minibatches (class default 10) on the same kernels --
    # the matrix-core epochs read the permutation in place, the row kernels of
    # csrc/pmlp.hip take gathered pieces
    agent.num_minibatchs = nmb
    assert agent.num_iterations == 0           # the first step is 1 = 1 mod 25
    # which implementation ran
    calls = {"direct": 0, "pmlp_critic": 0, "linear": 0}
    run = objective.BBDirectEpoch.run
    monkeypatch.setattr(objective.BBDirectEpoch, "run", lambda *a, **k: (
        calls.__setitem__("direct", calls["direct"] + 1), run(*a, **k))[1])
    cu = pmlp_ops.critic_update
    monkeypatch.setattr(pmlp_ops, "critic_update", lambda *a, **k: (
        calls.__setitem__("pmlp_critic", calls["pmlp_critic"] + 1),
        cu(*a, **k))[1])
    lin = mlp_ops._Linear.apply
    monkeypatch.setattr(mlp_ops._Linear, "apply", lambda *a: (
        calls.__setitem__("linear", calls["linear"] + 1), lin(*a))[1])
    hid = lambda h: [h[0]] * h[1]
    oracle = OracleBBRL(BB_MP, N, d_in, hid(cfg["policy_hidden"]),
                        hid(cfg["critic_hidden"]), cfg["act"], cfg["std_only"],
                        1e-5, 0.01, LR, EPOCHS, 0.005, 0.0005, 1.0, True,
                        clip_critic=cfg["clip_critic"], dtype=dt,
                        balance=balance, weight_decay=cfg["wd"],
                        num_minibatchs=nmb, episodes=episodes)
    with torch.no_grad():
        for po, pg in zip(oracle.pnet, agent.policy.mean_net.parameters()):
            po.copy_(pg.cpu())
        for po, pg in zip(oracle.cnet, agent.critic.net.parameters()):
            po.copy_(pg.cpu())
        oracle.var.copy_(agent.policy.variance_net.variable.cpu())
    resets, eps = _forced_state(N, 4, 20, dt, episodes, 3)
    _force_resets(agent.sampler.train_envs, resets, dt)
    _force_noise(agent.policy, eps)
    oracle.forced_reset, oracle.forced_eps = resets, eps
    captured = {}
    pd = agent.process_dataset

    def grab(ds):
        out = pd(ds)
        captured.update({k: v.detach().cpu() for k, v in out.items()
                         if torch.is_tensor(v) and k != "segment_params_L"})
        return out
    agent.process_dataset = grab
    np.random.seed(5)                       # (the minibatch permutations)
    res = dict(agent.step())
    np.random.seed(5)
    oracle.step()
    ref = oracle.last
    assert captured["segment_action"].shape[0] == N * episodes
    f64 = dt == torch.float64
    # float32: rounding of 128- / 256-term sums; float64: the basis table and the
    # projection's Newton iteration stop at 1e-10 .. 1e-12, Adam's first steps
    # (lr * g / (|g| + 1e-8)) amplify that in parameters with tiny gradients
    t = (lambda a, b: b) if f64 else (lambda a, b: a)
    _close("segment_action", captured["segment_action"], ref["segment_action"],
           t(3e-6, 1e-11))
    _close("segment_log_prob", captured["segment_log_prob"],
           ref["segment_log_prob"], t(4e-6, 1e-10))
    _close("segment_value", captured["segment_value"], ref["segment_value"],
           t(4e-6, 1e-11))
    _close("segment_reward", captured["segment_reward"], ref["segment_reward"],
           t(2e-6, 1e-10))
    _close("segment_advantage", captured["segment_advantage"],
           ref["segment_advantage"], t(1e-5, 1e-9))
    for pg, po in zip(agent.critic.net.parameters(), oracle.cnet):
        # (minibatches: nmb x the Adam steps, on 6-row pieces)
        _close("critic", pg.detach().cpu(), po.detach(),
               t(5e-6 * nmb, 1e-8 * nmb))
    for pg, po in zip(agent.policy.mean_net.parameters(), oracle.pnet):
        # (balance: 10 x the step size, twice the steps -- Adam's step is
        # lr * m / (sqrt(v) + eps), deviations scale with lr)
        _close("policy", pg.detach().cpu(), po.detach(),
               t(5e-5 if balance else 1e-5, 1e-7))
    _close("variance", agent.policy.variance_net.variable.detach().cpu(),
           oracle.var.detach(), t(5e-5 if balance else 1e-5, 1e-7))
    assert calls["direct"] == EPOCHS and calls["linear"] == 0
    # two hidden layers: the matrix-core epochs (csrc/mlpw_*.hip), one: pmlp
    rows = cfg["critic_hidden"][1] == 1
    assert calls["pmlp_critic"] == int(rows)
    assert agent._critic_path() == ("pmlp" if rows else "fused")
    _check_bbrl_metrics(res, oracle, t(2e-4, 1e-7), balance)
    if balance:
        assert np.array(oracle.balance_norms)[:, 1].max() > 0   # trust region active


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
def test_fused_objective_reports_the_same_metrics(ent_coef):
    """The fused policy objective (ONE C call, tce_policy_objective_*) and the
    op-by-op path return the same losses, KL diagnostics and gradient norm --
    also with an entropy bonus (its gradient is added inside the call)."""
    res = []
    for fused in (True, False):
        torch.manual_seed(3)
        agent, _ = build(64, 4, False, fused_policy_objective=fused,
                         graph_policy_update=fused,
                         entropy_penalty_coef=ent_coef)
        torch.manual_seed(5)
        res.append(agent.step())
    a, b = res
    keys = [k for k in b if k.startswith("projection_") and k.endswith("_mean")]
    keys += ["surrogate_loss_mean", "trust_region_loss_mean", "entropy_mean",
             "policy_loss_mean", "entropy_loss_mean", "policy_grad_norm_mean"]
    assert len(keys) >= 18
    for k in keys:
        if k == "projection_time":
            continue
        assert a[k] == pytest.approx(b[k], rel=2e-3, abs=2e-6), k


@pytest.mark.parametrize("minibatches", [None, ("numpy", 10), ("device", 10)])
def test_training_improves_reward_within_the_trust_region(minibatches):
    """A short training run on the synthetic reach-like task: the exploration
    reward rises steadily while every update stays inside the KL bounds --
    with the shipped YAMLs' one minibatch, and with the reference's class
    default of 10 (temporal_correlated_agent.py:25) on the fused minibatch
    epochs, permutations drawn by numpy on the host / by the device kernel."""
    from tce_rl_amd.config import tce_config
    from tce_rl_amd.mp_exp import MPExperiment
    cfg = tce_config("metaworld", num_env=256, num_basis=5, epochs=20,
                     evaluation_interval=0, iterations=40)
    if minibatches:
        a = cfg["params"]["agent"]["args"]
        a["minibatch_permutation"], a["num_minibatchs"] = minibatches
    exp = MPExperiment()
    exp.initialize(cfg, 0, None)
    rewards, covs, means = [], [], []
    for i in range(40):
        res = exp.iterate(cfg, 0, i)
        rewards.append(res["exploration_episode_reward_mean"])
        covs.append(res["projection_proj_old_cov_diff_max"])
        means.append(res["projection_proj_old_mean_diff_max"])
        assert np.isfinite(res["policy_loss_mean"])
    p = cfg["params"]["projection"]["args"]
    assert max(covs) <= p["cov_bound"] * 1.02
    assert max(means) <= p["mean_bound"] * 1.02
    assert np.mean(rewards[-5:]) > 0.6 * np.mean(rewards[:5])   # rewards are < 0
    assert rewards[-1] > rewards[0]
    if minibatches:
        assert tuple(exp.agent.last_critic_plan) == ("fused-narrow", 10, True,
                                                     True)


@pytest.mark.parametrize("shape", ["box_push", "table_tennis"])
def test_bbrl_midsize_training_improves_reward_within_the_trust_region(shape):
    """A short training run of the black-box agent with the reference's
    box-pushing / table-tennis nets (full covariance) on the hand-written
    epochs, lazy steps included: the exploration reward rises while every
    update stays inside the KL bounds, and iteration 26 -- the second one with
    the balance check -- reports its ratio."""
    c = BBRL_MID[shape]
    torch.manual_seed(0)
    agent, _ = build_bbrl(256, 20, c["policy_hidden"], c["critic_hidden"],
                          c["act"], c["std_only"], c["dtype"],
                          wd_policy=c["wd"], wd_critic=c["wd"],
                          lr_policy=1e-3, lr_critic=1e-3)
    agent.evaluation_interval = 0
    assert agent._critic_path() in ("fused", "pmlp")
    rewards, covs, means, ratios = [], [], [], {}
    for i in range(26):
        res = agent.step()
        rewards.append(res["exploration_segment_reward_mean"]
                       if "exploration_segment_reward_mean" in res
                       else res["exploration_episode_reward_mean"])
        covs.append(res["projection_proj_old_cov_diff_max"])
        means.append(res["projection_proj_old_mean_diff_max"])
        assert np.isfinite(res["policy_loss_mean"])
        if "balance_ratio" in res:
            ratios[i + 1] = res["balance_ratio"]
    assert agent._policy_path({"segment_params_L": agent.policy.policy(
        torch.zeros(2, agent.policy.mean_net.dim_in, device="cuda"))[1],
        "segment_state": torch.zeros(256, agent.policy.mean_net.dim_in,
                                     device="cuda")}) == "direct"
    assert sorted(ratios) == [1, 26]
    assert np.isfinite(ratios[26]) and ratios[26] > 0
    # the projection holds both bounds (build_bbrl: 0.005 / 0.0005)
    assert max(covs) <= 0.0005 * 1.02
    assert max(means) <= 0.005 * 1.02
    assert np.mean(rewards[-5:]) > np.mean(rewards[:5])          # rewards are < 0


OPTION_CASES = [
    dict(num_minibatchs=4),
    dict(clip_critic=0.5, clip_advantages=2.0, clip_grad_norm=0.5),
    dict(segment_advantage="accumulate", norm_advantages=False),
    dict(segment_advantage="accumulate", norm_advantages=True,
         clip_advantages=1.5),
    dict(segment_advantage="accumulated_rewards"),
    dict(use_gae=False, discount_factor=0.99),
    dict(set_variance=True, entropy_penalty_coef=0.01),
    dict(wd_policy=1e-3, wd_critic=1e-3),
    dict(_contextual=True),
    dict(_std_only=True),
    dict(_std_only=True, _contextual=True),
    dict(fused_policy_objective=False, graph_policy_update=True,
         overlap_updates=False),
    dict(balance_check=2),
]


@pytest.mark.parametrize("opts", OPTION_CASES, ids=lambda o: "-".join(o))
def test_agent_options_match_cpu_oracle(opts, monkeypatch):
    """Every agent / policy switch of the reference configs
    (temporal_correlated_agent.py:166-176 use_gae, :211-234 accumulate +
    norm / clip, :288-319 accumulated_rewards, :688-716 clipped value loss,
    util_data_structure.py:378-391 minibatches, abstract_policy.py:166-187
    contextual / std_only heads, set_variance, entropy penalty, weight decay,
    gradient clipping): TWO iterations of agent.step() against the CPU
    oracle with the same switches -- same rollout tensors, advantages and
    parameters, at the tolerance table of the default configuration (x 2 for
    the second iteration's accumulated Adam steps).  The second iteration
    also covers the LinearLR step and the variance set by set_variance."""
    from tce_rl_amd import critic_ops, mlp_ops
    opts = dict(opts)
    fused = opts.pop("fused_policy_objective", True)
    graph = opts.pop("graph_policy_update", False)
    overlap = opts.pop("overlap_updates", True)
    spy = _PathSpy(monkeypatch)
    mb_calls = []
    if "_contextual" in opts or "_std_only" in opts:
        mlp_ops.LIBRARY_CALLS.clear()
    if "num_minibatchs" in opts:
        orig = critic_ops.EpochRunner.epoch_minibatches

        def counted(self_, *a, **k):
            mb_calls.append(a[5])           # num_minibatches
            return orig(self_, *a, **k)
        monkeypatch.setattr(critic_ops.EpochRunner, "epoch_minibatches",
                            counted)
        mlp_ops.LIBRARY_CALLS.clear()
    agent, oracle, res = _agent_vs_oracle(overlap, fused, graph, "metaworld",
                                          5, iterations=2, rel_scale=2.0,
                                          **opts)
    if "_contextual" in opts or "_std_only" in opts:
        # the contextual covariance head (a second MLP,
        # abstract_policy.py:96-109) and the mean net's output layer run on
        # the generic dense layer of csrc/glin.hip under autograd
        assert not mlp_ops.LIBRARY_CALLS, dict(mlp_ops.LIBRARY_CALLS)
        want = "op_by_op" if "_contextual" in opts else "direct"
        assert agent.last_policy_plan.kind == want
        assert agent.last_critic_plan.kind == "fused-narrow"
    if "num_minibatchs" in opts:
        # the reference's minibatched critic update
        # (temporal_correlated_agent.py:343-366; class default 10) on the
        # hand-written epochs -- 3 epochs x 2 iterations, ONE C call each, the
        # policy epochs on DirectEpoch, no library GEMM, no autograd gather
        assert mb_calls == [opts["num_minibatchs"]] * 6
        assert (spy.direct, spy.node) == (6, 0)
        # ... and the agent's own named plans say the same (rl/tce_agent.py:
        # critic_plan / policy_plan are THE path selection)
        assert tuple(agent.last_critic_plan) == (
            "fused-narrow", opts["num_minibatchs"], True, True)
        assert agent.last_policy_plan.kind == "direct"
        assert not mlp_ops.LIBRARY_CALLS, dict(mlp_ops.LIBRARY_CALLS)
    for k in ("critic_loss_mean", "surrogate_loss_mean", "policy_loss_mean",
              "entropy_mean", "trust_region_loss_mean",
              "projection_proj_old_cov_diff_mean", "policy_grad_norm_mean",
              "exploration_segment_advantage_mean"):
        assert np.isfinite(res[k]), k
    lr = lambda opt: opt.param_groups[0]["lr"]
    assert lr(agent.policy_optimizer) == pytest.approx(lr(oracle.p_opt),
                                                       rel=1e-12)
    assert lr(agent.critic_optimizer) == pytest.approx(lr(oracle.c_opt),
                                                       rel=1e-12)


@pytest.mark.parametrize("critic_arith", ["f32", "bf16x3"])
def test_full_size_step_is_repeatable_and_inside_the_trust_region(critic_arith):
    """BASELINE configs[1] at full size (4096 envs, T 500, 50 + 50 epochs), the
    size-independent properties: two runs from the same seeds end bit-identical
    (every reduction has a fixed order, also with the critic, the policy and
    the K x K kernels on three streams), the projected policy stays inside the
    KL bounds and nothing is non-finite.  The adaptive critic split is off:
    it picks, from measured times, how many critic epochs run on 224 instead
    of 256 workgroups, and the number of per-workgroup gradient slabs is part
    of the summation order (float32 rounding, not repeatable bit for bit)."""
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        agent, cfg = build(4096, 50, True, num_basis=5,
                           adaptive_critic_split=False, critic_arith=critic_arith)
        torch.manual_seed(12)
        res = [agent.step() for _ in range(2)][-1]
        runs.append((res, to_cpu_params(agent.policy.mean_net),
                     to_cpu_params(agent.critic.net),
                     agent.policy.variance_net.variable.detach().cpu().clone()))
        del agent
    (ra, pa, ca, va), (rb, pb, cb, vb) = runs
    for x, y in zip(pa + ca + [va], pb + cb + [vb]):
        assert torch.equal(x, y)
    p = cfg["params"]["projection"]["args"]
    assert ra["projection_proj_old_cov_diff_max"] <= p["cov_bound"] * 1.02
    assert ra["projection_proj_old_mean_diff_max"] <= p["mean_bound"] * 1.02
    for k, v in ra.items():
        if isinstance(v, float):
            assert np.isfinite(v), k
    assert ra["num_global_steps"] == 2 * 4096 * 500


@pytest.mark.parametrize("env,N,nb,dtype", [
    ("box_push", 8192, 8, "float64"),            # BASELINE configs[2] as the reference runs it
    ("table_tennis", 4096, 8, "float32"),        # configs[4], one GPU's shard, K 63
    ("table_tennis", 4096, 3, "float32")])       # ... with the reference's 3 basis functions
def test_full_size_steps_of_the_other_configs(env, N, nb, dtype):
    """BASELINE configs[2] and [4] at their stated env counts (per GPU), the
    size-independent properties test_full_size_step_... checks for configs[1]:
    two runs from the same seeds end bit-identical, the projected policy stays
    inside the KL bounds, nothing is non-finite, the step count is N x T x
    iterations.  (50 + 50 epochs like the benchmark would take a minute per
    case in float64: 6 + 6 epochs exercise the same launches.)"""
    runs = []
    T = {"box_push": 100, "table_tennis": 350}[env]
    for _ in range(2):
        torch.manual_seed(11)
        agent, cfg = build(N, 6, True, env=env, num_basis=nb, dtype=dtype,
                           adaptive_critic_split=False)
        torch.manual_seed(12)
        res = [agent.step() for _ in range(2)][-1]
        runs.append((res, to_cpu_params(agent.policy.mean_net),
                     to_cpu_params(agent.critic.net),
                     agent.policy.variance_net.variable.detach().cpu().clone()))
        del agent
        torch.cuda.empty_cache()
    (ra, pa, ca, va), (rb, pb, cb, vb) = runs
    for x, y in zip(pa + ca + [va], pb + cb + [vb]):
        assert torch.equal(x, y)
    p = cfg["params"]["projection"]["args"]
    assert ra["projection_proj_old_cov_diff_max"] <= p["cov_bound"] * 1.02
    assert ra["projection_proj_old_mean_diff_max"] <= p["mean_bound"] * 1.02
    for k, v in ra.items():
        if isinstance(v, float):
            assert np.isfinite(v), k
    assert ra["num_global_steps"] == 2 * N * T


def test_full_size_bbrl_shard_is_repeatable():
    """BASELINE configs[3], one GPU's 4096-env shard, the reference's 100 + 100
    epochs (mprl/config/metaworld/bbrl/entire/shared.yaml:38-39): two runs end
    bit-identical (fixed slab order in csrc/smlp.hip), nothing is non-finite,
    the variance set from the projection stays positive."""
    from tce_rl_amd.config import bbrl_config
    from tce_rl_amd.mp_exp import MPExperiment
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        cfg = bbrl_config(num_env=4096, epochs=100)
        exp = MPExperiment()
        exp.initialize(cfg, 0, None)
        agent = exp.agent
        torch.manual_seed(12)
        res = [agent.step() for _ in range(2)][-1]
        runs.append((res, to_cpu_params(agent.policy.mean_net),
                     to_cpu_params(agent.critic.net),
                     agent.policy.variance_net.variable.detach().cpu().clone()))
        del agent, exp
    (ra, pa, ca, va), (rb, pb, cb, vb) = runs
    for x, y in zip(pa + ca + [va], pb + cb + [vb]):
        assert torch.equal(x, y)
    for k, v in ra.items():
        if isinstance(v, float):
            assert np.isfinite(v), k
    assert ra["num_global_steps"] == 2 * 4096 * 500
    assert np.isfinite(ra["projection_kl"]) and ra["projection_entropy"] != 0


_RESOLVED = sorted(f[:-5] for f in __import__("os").listdir(
    __import__("os").path.join(__import__("os").path.dirname(
        __import__("os").path.abspath(__file__)), "golden", "resolved")))


@pytest.mark.parametrize("doc", _RESOLVED)
def test_step_from_the_references_resolved_documents(doc):
    """f3: the reference's own experiment documents (every
    mprl/config/<task>/<tcp|bbrl>/entire/local.yaml resolved against its
    shared.yaml; VALUES committed under tests/golden/resolved/ by
    make_resolved_cfg.py) drive MPExperiment + agent.step() on the GPU, one
    per task family and agent type.  Changed for the run: the env count (the
    reference's 4 .. 38 MuJoCo processes -> 32 synthetic envs), the epochs
    (2 + 2), the task metric names (the synthetic suite reports `success`) and
    -- black-box documents, whose MP block leaves the phase / basis constants
    to fancy_gym's defaults -- those constants."""
    import json
    import os
    from tce_rl_amd.mp_exp import MPExperiment, dim_policy_out
    here = os.path.dirname(os.path.abspath(__file__))
    d = json.load(open(os.path.join(here, "golden", "resolved", doc + ".json")))
    p = d["params"]
    for blk in p.values():
        blk["args"]["device"] = "cuda"
    sa = p["sampler"]["args"]
    sa.update(num_env_train=32, num_env_test=8, task_specified_metrics=["success"])
    p["agent"]["args"].update(epochs_policy=2, epochs_critic=2,
                              evaluation_interval=0)
    fam = "TableTennis" if "TableTennis" in sa["env_id"] else \
        "BoxPushing" if "BoxPushing" in sa["env_id"] else \
        "HopperJump" if "HopperJump" in sa["env_id"] else "metaworld"
    defaults = {"metaworld": dict(alpha=10, dt=0.0125, tau=5.0),
                "BoxPushing": dict(alpha=10, dt=0.02, tau=2.0),
                "TableTennis": dict(alpha=25, dt=0.008, tau=0.75),
                "HopperJump": dict(alpha=25, dt=0.008, tau=2.0)}[fam]
    for k, v in dict(defaults, alpha_phase=3, basis_bandwidth_factor=3,
                     dtype=p["agent"]["args"]["dtype"],
                     device="cuda").items():
        p["mp"]["args"].setdefault(k, v)
    if "mp" in sa:
        sa["mp"] = p["mp"]
    if "mp" in p["policy"]["args"]:
        p["policy"]["args"]["mp"] = p["mp"]
    cfg = {"name": d["name"], "seed": 0, "iterations": d["iterations"],
           "params": p}
    torch.manual_seed(0)
    exp = MPExperiment()
    exp.initialize(cfg, 0, None)
    agent = exp.agent
    assert agent.policy.dim_out == dim_policy_out(p)
    assert type(agent).__name__ == p["agent"]["type"]
    # several episodes per env (5 in three of the documents, 2 in one): the
    # dataset the agent works on has one row per env AND episode, and every
    # one of those episodes is counted in the env steps
    episodes = int(sa.get("episodes_per_train_env", 1))
    assert agent.sampler.episodes_per_train_env == episodes
    rows = []
    pd = agent.process_dataset
    agent.process_dataset = lambda ds: (
        rows.append(ds["segment_state"].shape[0]), pd(ds))[1]
    T = agent.sampler.train_envs.num_times
    for it in range(2):
        res = agent.step()
        assert agent.num_global_steps == (it + 1) * 32 * episodes * T
        assert res["num_global_steps"] == agent.num_global_steps
    assert rows == [32 * episodes] * 2
    for k in ("critic_loss_mean", "surrogate_loss_mean", "policy_loss_mean",
              "trust_region_loss_mean", "entropy_mean"):
        assert np.isfinite(res[k]), k
    for q in agent.policy.parameters + agent.critic.parameters:
        assert torch.isfinite(q).all()
    want = torch.float64 if "64" in str(p["agent"]["args"]["dtype"]) \
        else torch.float32
    assert agent.policy.parameters[0].dtype == want


def test_objective_on_one_stream_equals_two_streams(monkeypatch):
    """tce_policy_objective_streams(1) -- what a sharded run uses, where the
    second stream would share a hardware queue with the critic's -- runs the
    same kernels in one stream order: bit-identical parameters."""
    out = []
    for n in ("1", "2"):
        monkeypatch.setenv("TCE_OBJECTIVE_STREAMS", n)
        torch.manual_seed(21)
        agent, _ = build(256, 4, True, adaptive_critic_split=False)
        torch.manual_seed(22)
        agent.step()
        out.append(to_cpu_params(agent.policy.mean_net) +
                   [agent.policy.variance_net.variable.detach().cpu().clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("env,nb,dtype,balance", [
    ("metaworld", 5, "float32", None), ("box_push", 8, "float64", None),
    ("table_tennis", 3, "float32", None), ("metaworld", 5, "float32", 2)])
def test_fused_epoch_tail_is_bit_identical(env, nb, dtype, balance):
    """policy_tail_kernel (join add + Cholesky head backward + clip + Adam +
    record in one launch) == the five launches it replaces
    (tce_policy_tail_fused(0)): parameters, both moments, the optimizer's state
    vector and the record rows after two iterations, bit for bit -- on the
    128 x 2 float32 kernels, both pmlp families and a balance-check iteration."""
    from tce_rl_amd import _lib
    lib = _lib.load()
    out = []
    try:
        for on in (1, 0):
            lib.tce_policy_tail_fused(on)
            torch.manual_seed(31)
            agent, _ = build(96, 4, True, env=env, num_basis=nb, dtype=dtype,
                             adaptive_critic_split=False,
                             balance_check=balance)
            torch.manual_seed(32)
            res = [dict(agent.step()) for _ in range(2)]
            opt = agent.policy_optimizer
            out.append(([t.clone() for t in (opt.flat_param, opt.m, opt.v,
                                             opt.dev_state)], res))
    finally:
        lib.tce_policy_tail_fused(1)
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    for ra, rb in zip(out[0][1], out[1][1]):
        for k in ("surrogate_loss_mean", "trust_region_loss_mean",
                  "policy_grad_norm_mean", "entropy_mean"):
            if k in ra:
                assert ra[k] == rb[k], k


def test_deferred_join_does_not_depend_on_side_stream_timing(monkeypatch):
    """The trust-region gradient w.r.t. the mean is written by a kernel on the
    library's second stream and added to on the caller's stream in the
    deferred-join form of tce_policy_objective_* (what DirectEpoch.run uses).
    With the second stream stalled at the top of every epoch (a long sleep
    kernel in front of the covariance projection) the parameters must still
    be bit-identical to the one-stream order -- ordering by events, not by
    luck."""
    import ctypes
    from tce_rl_amd import _lib
    from tce_rl_amd.rl import objective
    out = []
    for mode in ("one", "stalled"):
        monkeypatch.setenv("TCE_OBJECTIVE_STREAMS",
                           "1" if mode == "one" else "2")
        torch.manual_seed(21)
        agent, _ = build(256, 4, False, adaptive_critic_split=False)
        if mode == "stalled":
            h = ctypes.c_void_p()
            _lib.call("tce_policy_objective_side_stream", ctypes.byref(h))
            side = torch.cuda.ExternalStream(h.value)
            orig = objective.begin

            def begin(*a, **kw):
                orig(*a, **kw)
                # behind the projection forward, in front of kl_shared
                with torch.cuda.stream(side):
                    torch.cuda._sleep(20_000_000)      # ~10 ms
            monkeypatch.setattr(objective, "begin", begin)
        torch.manual_seed(22)
        agent.step()
        out.append(to_cpu_params(agent.policy.mean_net) +
                   [agent.policy.variance_net.variable.detach().cpu().clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


TIME_KEYS = ("sampling_time", "process_dataset_time", "update_time",
             "update_critic_time", "update_policy_time", "projection_time",
             "policy_epochs_device_time", "evaluation_time")


@pytest.mark.parametrize("kind", ["tce", "bbrl"])
def test_lazy_step_equals_eager_step(kind):
    """step() hands its metrics back as util.LazyMetrics and does not wait for
    the device (agent.lazy_metrics, the default): three iterations with the
    metrics read only at the end leave bit-identical parameters and the same
    metrics (timers aside) as three iterations that read them at once."""
    from tce_rl_amd.util import LazyMetrics
    out = []
    for lazy in (False, True):
        torch.manual_seed(31)
        np.random.seed(31)
        if kind == "tce":
            agent, _ = build(64, 3, True, lazy_metrics=lazy)
            nets = [agent.policy.mean_net, agent.critic.net]
        else:
            agent, _ = build_bbrl(64, 3)
            agent.lazy_metrics = lazy
            agent.evaluation_interval = 0     # (an evaluation reads the metrics)
            nets = [agent.policy.mean_net, agent.critic.net]
        torch.manual_seed(32)
        results = [agent.step() for _ in range(3)]
        if lazy:
            # (the first BBRL iteration latches the initial entropy and is eager)
            assert all(isinstance(r, LazyMetrics) for r in results[1:])
            assert results[-1].pending
        else:
            assert not any(isinstance(r, LazyMetrics) and r.pending for r in results)
        params = sum((to_cpu_params(n) for n in nets), []) + \
            [agent.policy.variance_net.variable.detach().cpu().clone()]
        out.append((params, [dict(r) for r in results]))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)
    for ra, rb in zip(out[0][1], out[1][1]):
        assert set(ra) == set(rb)
        for k in ra:
            if k not in TIME_KEYS:
                # (the gradient-norm records sum squares with float atomics:
                # equal to the last bits, not bit for bit)
                tol = 1e-3 if "grad_norm" in k else 0.0   # (std of 3 near-equal values)
                same = ra[k] == rb[k] or (ra[k] != ra[k] and rb[k] != rb[k]) or \
                    abs(ra[k] - rb[k]) <= tol * max(abs(ra[k]), abs(rb[k]))
                assert same, (k, ra[k], rb[k])
