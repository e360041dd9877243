"""The ProDMP trajectory and pair log-prob kernels over the WHOLE family of
shapes their entry points accept (num_dof 1..8, num_basis + 1 = 1..16, any
horizon, env count and pair count), against the float64 CPU oracle.

tests/test_prodmp_gpu.py pins the four shipped (dof, basis) shapes at their own
horizons; the kernels pick their code path from those numbers (compile-time or
run-time basis count, 16- / 8-byte / scalar row stores, envs side by side in a
workgroup, parameters staged 32 envs at a time, register or LDS pair kernels,
envs and waves per block from the LDS budget), so every path is run here at
the sizes where such arithmetic goes wrong: first / last of a range, ragged
last groups, second loop iterations, and the bytes just outside the output."""
import itertools

import pytest
import torch

from oracle import tce_oracle as O
from oracle.prodmp_oracle import ProDMPOracle, pair_log_prob
from prodmp_cases import affine, inputs, make
from test_prodmp_gpu import LOGP_REL

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

# MP constants of the shipped documents (tests/golden/resolved/*.json,
# tce_rl_amd/config); t_max: the longest horizon (0.2 of init-time spread
# included) inside the pre-computed range delay + 5 tau
MPC = {
    "hopper": dict(tau=0.8, alpha_phase=3, alpha=10, dt=0.008,
                   basis_bandwidth_factor=3, weights_scale=1, goal_scale=1,
                   relative_goal=False),
    "metaworld": dict(tau=5, alpha_phase=3, alpha=10, dt=0.0125,
                      basis_bandwidth_factor=5, weights_scale=0.1,
                      goal_scale=0.1, relative_goal=True),
    "box_push": dict(tau=2.0, alpha_phase=3, alpha=10, dt=0.02,
                     basis_bandwidth_factor=3, weights_scale=0.3,
                     goal_scale=0.3, relative_goal=False),
    "table_tennis": dict(tau=0.75, delay=0.3, alpha_phase=3, alpha=25,
                         dt=0.008, basis_bandwidth_factor=3, weights_scale=0.7,
                         goal_scale=0.1, relative_goal=True),
}
_CONSTS_OF_DOF = {1: "box_push", 2: "table_tennis", 3: "hopper",
                  4: "metaworld", 5: "table_tennis", 6: "hopper",
                  7: "box_push", 8: "metaworld"}


def cfg_of(dof, nbg, T, consts=None, flip_goal=False):
    """Config dict of a (dof, num_basis + 1) shape on shipped MP constants
    (hopper's for dof 3); a horizon beyond their range takes Metaworld's."""
    c = dict(MPC[consts or _CONSTS_OF_DOF[dof]])
    if T * c["dt"] + 0.2 > c.get("delay", 0.0) + 5 * c["tau"]:
        c = dict(MPC["metaworld"])
    if flip_goal:
        c["relative_goal"] = not c["relative_goal"]
    return dict(c, num_dof=dof, num_basis=nbg - 1)


@pytest.fixture(scope="module")
def ops():
    from tce_rl_amd import ops
    return ops


# ---------------------------------------------------------------------------
# A. trajectories
# ---------------------------------------------------------------------------
SENTINEL = -7777.25
GUARD, TAIL = 64, 8192


def guarded(N, T, C, dtype):
    """An output tensor inside a larger buffer filled with a sentinel: the wave
    slabs of the kernels leave as whole chunks counted by `nvalid`, and a wrong
    count writes past the end without changing any compared value."""
    n = N * T * C
    buf = torch.full((GUARD + n + TAIL,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(N, T, C)


def assert_guards_untouched(buf, n, what):
    assert bool((buf[:GUARD] == SENTINEL).all()), what + ": wrote before out"
    tail = buf[GUARD + n:] != SENTINEL
    assert not bool(tail.any()), "%s: wrote %d elements past the end, first " \
        "at +%d" % (what, int(tail.sum()), int(tail.nonzero()[0]))


def _traj_case(ops, cfg, dtype, N, T, seed=1):
    """Three ways into the kernels -- tagged uniform grid (rows kernel for dof
    3, 4, 5, 7), untagged copy of it (general kernel, per-element basis),
    differing init times (general kernel by the device flag) -- each into a
    guarded output, against oracle.sample_trajectories."""
    mp, oracle = make(cfg, dtype)
    C = 2 * cfg["num_dof"]
    tol = 2e-5 if dtype == F32 else 1e-10
    wtol = 1e-5 if dtype == F32 else 1e-12
    mean, L, eps, t0d, y0, v0 = inputs(cfg, N, dtype, seed, False)
    w = ops.mvn_rsample(mean.cuda(), L.cuda(), eps.cuda())
    K = mean.shape[1]                 # up to 128 terms per sum (the shipped 63)
    torch.testing.assert_close(w.cpu(), O.mvn_rsample(mean, L, eps),
                               rtol=wtol, atol=wtol * max(1.0, K / 64))
    for way in ("rows", "general", "init_times"):
        t0 = t0d if way == "init_times" else torch.zeros_like(t0d)
        times_cpu = O.get_times(t0, cfg["dt"], T)
        if way != "general":
            tg = ops.times(t0.cuda(), cfg["dt"], T)
            torch.testing.assert_close(tg.cpu(), times_cpu, rtol=3e-7,
                                       atol=2e-7)
            pos, vel = oracle.sample_trajectories(times_cpu, mean, L, t0, y0,
                                                  v0, eps)
            ref = torch.cat([pos, vel], -1)
        tg = affine(times_cpu)
        if way == "general":
            tg = tg.clone()
        buf, out = guarded(N, T, C, dtype)
        got = ops.prodmp_traj(mp, tg, w, t0.cuda(), y0.cuda(), v0.cuda(),
                              out=out)
        assert got.data_ptr() == out.data_ptr()
        what = "%s dof %d nbg %d T %d N %d" % (way, cfg["num_dof"],
                                                 cfg["num_basis"] + 1, T, N)
        assert_guards_untouched(buf, N * T * C, what)
        torch.testing.assert_close(out, ref.cuda(), rtol=tol, atol=tol,
                                   msg=lambda m: what + ": " + m)


TS = [1, 2, 17, 63, 64, 65, 86, 100, 127, 128, 129, 250, 256, 257, 700]
NS = [1, 2, 3, 31, 32, 33, 257]
NBGS = [1, 4, 5, 6, 9, 11, 16]


def _ragged_n(i, T):
    """An env count of NS, by turns, that does not fill the last group of the
    256 // T envs a workgroup of the rows kernel puts side by side."""
    spb = 256 // T if T <= 128 else 1
    for k in range(len(NS)):
        N = NS[(i + k) % len(NS)]
        if spb == 1 or N % spb:
            return N
    raise AssertionError(T)


# every dof with every basis count of NBGS: each compile-time specialisation
# ((4,5) (4,6) (4,9) (7,4) (7,9)) and its run-time siblings; 15 horizons and 7
# env counts by turns
_SHAPE_CASES = [
    (dof, nbg, TS[(2 * i + 7) % len(TS)], NS[(i + i // 7) % len(NS)],
     i % 3 == 0)
    for i, (dof, nbg) in enumerate(itertools.product(range(1, 9), NBGS))]


# both dtypes where the basis count picks a kernel (dof 4, 7), by turns elsewhere
_SHAPE_DTYPES = [c + (dt,) for i, c in enumerate(_SHAPE_CASES)
                 for dt in ((F32, F64) if c[0] in (4, 7) else
                            (F32,) if (i + c[0]) % 2 else (F64,))]


@pytest.mark.parametrize("dof,nbg,T,N,flip,dtype", _SHAPE_DTYPES)
def test_traj_every_shape_vs_oracle(ops, dof, nbg, T, N, flip, dtype):
    consts = "table_tennis" if dof == 7 and nbg % 2 == 0 else None
    _traj_case(ops, cfg_of(dof, nbg, T, consts, flip), dtype, N, T)


# the rows kernel's dofs at every horizon edge: T < 64, 64 / 65, 86 (256 // T
# leaves dead lanes), 128 / 129 (last packed / first unpacked), 256 / 257
# (second blockIdx.x), with an env count that leaves the last group ragged;
# the basis count alternates between a specialised one and its sibling
_T_NBG = {3: (4, 4), 4: (6, 7), 5: (5, 9), 7: (9, 8)}
_T_CASES = [(dof, _T_NBG[dof][j % 2], T, _ragged_n(j + dof, T))
            for dof in (3, 4, 5, 7) for j, T in enumerate(TS)]


# both dtypes at the horizons where the packing changes, by turns elsewhere
_T_BOTH = (2, 17, 64, 65, 86, 128, 129, 257)
_T_DTYPES = [c + (dt,) for i, c in enumerate(_T_CASES)
             for dt in ((F32, F64) if c[2] in _T_BOTH else
                        (F32,) if i % 2 else (F64,))]


@pytest.mark.parametrize("dof,nbg,T,N,dtype", _T_DTYPES)
def test_traj_horizon_edges_vs_oracle(ops, dof, nbg, T, N, dtype):
    _traj_case(ops, cfg_of(dof, nbg, T), dtype, N, T, seed=2)


_N_TS = [86, 17, 100, 64, 2, 128, 65]
_N_CASES = [(dof, _T_NBG[dof][(j + 1) % 2], _N_TS[(j + dof) % 7], N)
            for dof in (3, 4, 5, 7) for j, N in enumerate(NS)] + \
    [(dof, 3, 100, N) for dof in (1, 2, 6, 8) for N in (33, 257)]


@pytest.mark.parametrize("dof,nbg,T,N", _N_CASES)
def test_traj_env_count_edges_vs_oracle(ops, dof, nbg, T, N):
    _traj_case(ops, cfg_of(dof, nbg, T), F32 if (dof + N) % 2 else F64, N, T,
               seed=3)


def test_ragged_case_tables_cover_what_they_claim():
    """The case tables above: every horizon with envs side by side meets an env
    count that does not fill the last group, and one that does."""
    for dof in (3, 4, 5, 7):
        for T in TS:
            if T > 128:
                continue
            spb = 256 // T
            ns = [c[3] for c in _T_CASES + _N_CASES + [
                s[:1] + (0,) + s[2:4] for s in _SHAPE_CASES]
                if c[0] == dof and c[2] == T]
            assert any(n % spb for n in ns), (dof, T)
    assert {(c[0], c[1]) for c in _SHAPE_CASES} >= {
        (7, 9), (7, 4), (7, 11), (4, 6), (4, 9), (4, 5), (4, 11), (5, 5),
        (3, 4)} | {(d, 16) for d in range(1, 9)}


# one case per store shape (8-byte chunks at 24-byte rows, 16-byte chunks,
# 8-byte chunks at 40-byte rows) in which a workgroup of the rows kernel owns
# MORE than the 32 envs it stages at a time: envs per workgroup =
# N * ceil(T / 256) // 2048 rounded up to the side-by-side count
_MANY = [(3, 4, 100, 70001, 34), (4, 6, 257, 34001, 33), (5, 6, 64, 70003, 36)]


@pytest.mark.parametrize("dof,nbg,T,N,epr", _MANY)
def test_traj_second_staged_chunk_of_many_envs(ops, dof, nbg, T, N, epr):
    dtype = F32
    cfg = cfg_of(dof, nbg, T)
    mp, oracle = make(cfg, dtype)
    spb = 256 // T if T <= 128 else 1
    txr = 1 if spb > 1 else -(-T // 256)
    want = -(-max(spb, N * txr // 2048) // spb) * spb
    assert want == epr > 32, (want, epr)         # the launch arithmetic read
    K, C = dof * nbg, 2 * dof
    g = torch.Generator().manual_seed(dof)
    w = 0.5 * torch.randn(N, K, generator=g, dtype=dtype)
    y0 = torch.rand(N, dof, generator=g, dtype=dtype) * 2 - 1
    v0 = 0.1 * torch.randn(N, dof, generator=g, dtype=dtype)
    t0 = torch.zeros(N, dtype=dtype)
    tg = affine(O.get_times(t0, cfg["dt"], T))
    buf, out = guarded(N, T, C, dtype)
    ops.prodmp_traj(mp, tg, w.cuda(), t0.cuda(), y0.cuda(), v0.cuda(), out=out)
    assert_guards_untouched(buf, N * T * C, "dof %d" % dof)
    assert bool(torch.isfinite(out).all())
    assert not bool((out == SENTINEL).any())      # every element was written
    # envs on both sides of every 32-env staging boundary and of the workgroup
    # boundaries of a few workgroups (first two, a middle one, the last two)
    nwg = -(-N // epr)
    pick = {0, N - 1}
    for by in (0, 1, nwg // 2, nwg - 2, nwg - 1):
        b = by * epr
        pick |= {b - 1, b, b + 1, b + 31, b + 32, b + 33, b + epr - 1}
    idx = torch.tensor(sorted(n for n in pick if 0 <= n < N))
    times_cpu = O.get_times(t0[idx], cfg["dt"], T)
    pos, vel = oracle.traj(times_cpu, w[idx], t0[idx], y0[idx], v0[idx])
    torch.testing.assert_close(out[idx.cuda()].cpu(), torch.cat([pos, vel], -1),
                               rtol=2e-5, atol=2e-5)
    # ... and a strided sample of the rest: each env's own parameters
    idx = torch.arange(7, N, 997)
    times_cpu = O.get_times(t0[idx], cfg["dt"], T)
    pos, vel = oracle.traj(times_cpu, w[idx], t0[idx], y0[idx], v0[idx])
    torch.testing.assert_close(out[idx.cuda()].cpu(), torch.cat([pos, vel], -1),
                               rtol=2e-5, atol=2e-5)


def test_traj_refuses_shapes_outside_the_family(ops):
    """num_dof > 8 / num_basis + 1 > 16 have no kernel: refused by name, both
    by the MP constructor and by the C entry."""
    from tce_rl_amd._lib import call
    from tce_rl_amd.mp import ProDMP
    for dof, nbg in ((9, 4), (4, 17)):
        with pytest.raises(NotImplementedError, match="num_basis <= 15"):
            ProDMP(dtype=F32, device="cuda",
                   **cfg_of(dof, nbg, 100, "metaworld"))
    mp = ProDMP(dtype=F32, device="cuda", **cfg_of(4, 6, 100))
    p = torch.zeros(64, device="cuda").data_ptr()
    a = list(mp.c_args())
    tail = lambda dof: (p, 0, p, p, p, p, p, p, p, 1, 4, dof, None)
    with pytest.raises(RuntimeError, match="num_dof must be <= 8"):
        call("tce_prodmp_traj_f32", *a, *tail(9))
    a[2] = 17
    with pytest.raises(RuntimeError, match=r"num_basis \+ 1 must be <= 16"):
        call("tce_prodmp_traj_f32", *a, *tail(4))


# ---------------------------------------------------------------------------
# B. pair log-prob, forward and backward
# ---------------------------------------------------------------------------
def hand_pairs(T, P, seed=0):
    """Pair lists with what get_time_pairs never draws: a pair starting at step
    0, one ending at T - 1, adjacent steps, the whole horizon, pairs sharing a
    start and pairs sharing an end point; filled up with seeded random i < j."""
    edge = [(0, T - 1), (0, 1), (T - 2, T - 1), (1, T - 1), (0, T // 2),
            (T // 2, T // 2 + 1), (T // 2, T - 1)]
    if P == 1:
        edge = edge[seed % 3:]
    g = torch.Generator().manual_seed(100 + seed)
    while len(edge) < P:
        i, j = sorted(torch.randint(0, T, (2,), generator=g).tolist())
        if i < j:
            edge.append((i, j))
    return torch.tensor(edge[:P], dtype=torch.long)


def drawn_pairs(T, seed):
    torch.manual_seed(seed)
    return O.get_time_pairs(T, dict(num_select=25, fixed_interval=True))


def _pairs(T, kind, seed):
    return drawn_pairs(T, seed) if kind == "draw" else hand_pairs(T, kind, seed)


def oracle_logp_and_grads(oracle, traj, mean, L, shared, times, t0, y0, v0,
                          pairs, dloss):
    """log-probs [N, P] of the oracle and, through autograd, the gradients of
    sum_n dloss(logp[n], n-slice) w.r.t. the mean [N, K] and the factor ([K, K]
    shared, [N, K, K] per env).  Envs go through in slices so that the
    [n, P, K, K] covariances of the restatement stay small."""
    N, K = mean.shape
    P = pairs.shape[0]
    m = mean.clone().requires_grad_(True)
    Lb = (L[0] if shared else L).clone().requires_grad_(True)
    step = max(1, min(N, int(3e6 // (P * K * K)) or 1))
    out = []
    for a in range(0, N, step):
        sl = slice(a, min(N, a + step))
        n = sl.stop - sl.start
        Ls = Lb[None].expand(n, -1, -1) if shared else Lb[sl]
        lp = pair_log_prob(oracle, traj[sl], m[sl], Ls, times[sl], t0[sl],
                           y0[sl], v0[sl], pairs)
        dloss(lp, sl).backward()
        out.append(lp.detach())
    return torch.cat(out), m.grad, torch.tril(Lb.grad)


def _gpu_logp_and_grads(ops, mp, traj, mean, L, shared, tg, t0, y0, v0, pairs,
                        wgt):
    N = mean.shape[0]
    m_g = mean.cuda().requires_grad_(True)
    Lb_g = (L[0] if shared else L).cuda().requires_grad_(True)
    L_g = ops.expand_shared(Lb_g, N) if shared else Lb_g
    lp = ops.pair_log_prob(mp, traj.cuda(), m_g, L_g, tg, t0.cuda(), y0.cuda(),
                           v0.cuda(), pairs.cuda())
    (lp * wgt.cuda()).sum().backward()
    return lp.detach().cpu(), m_g.grad.cpu(), torch.tril(Lb_g.grad.cpu())


def _pair_setup(cfg, T, N, dtype, shared, uniform_t0, seed=3):
    mp, oracle = make(cfg, dtype)
    mean, L, eps, t0, y0, v0 = inputs(cfg, N, dtype, seed, uniform_t0)
    if shared:
        L = L[:1].expand(N, -1, -1).contiguous()
    times_cpu = O.get_times(t0, cfg["dt"], T)
    pos, vel = oracle.sample_trajectories(times_cpu, mean, L, t0, y0, v0, eps)
    return mp, oracle, mean, L, t0, y0, v0, times_cpu, torch.cat([pos, vel], -1)


def _pair_case(ops, dof, nbg, T, N, pkind, shared=True, uniform_t0=True,
               static=True, budgets=(0,), consts=None, seed=3):
    """The body of test_prodmp_gpu._pair_logprob_fwd_bwd_vs_oracle (float64,
    1e-8 forward / 1e-7 backward) for any shape, env count and pair list; every
    CU budget in `budgets` against the oracle, each launched twice: bit-equal."""
    from tce_rl_amd._lib import call
    cfg = cfg_of(dof, nbg, T, consts)
    mp, oracle, mean, L, t0, y0, v0, times_cpu, traj = _pair_setup(
        cfg, T, N, F64, shared, uniform_t0, seed)
    pairs = _pairs(T, pkind, seed)
    wgt = torch.randn(N, pairs.shape[0], dtype=F64,
                      generator=torch.Generator().manual_seed(seed))
    lp_ref, gm_ref, gl_ref = oracle_logp_and_grads(
        oracle, traj, mean, L, shared, times_cpu, t0, y0, v0, pairs,
        lambda lp, sl: (lp * wgt[sl]).sum())
    tg = affine(times_cpu)
    what = "dof %d nbg %d T %d N %d P %d" % (dof, nbg, T, N, pairs.shape[0])
    call("tce_pair_env_static", int(static))
    try:
        for budget in budgets:
            call("tce_set_cu_budget", budget)
            runs = [_gpu_logp_and_grads(ops, mp, traj, mean, L, shared, tg, t0,
                                        y0, v0, pairs, wgt) for _ in range(2)]
            lp, gm, gl = runs[0]
            msg = lambda m: "%s budget %d: %s" % (what, budget, m)
            torch.testing.assert_close(lp, lp_ref, rtol=1e-8, atol=1e-8, msg=msg)
            torch.testing.assert_close(gm, gm_ref, rtol=1e-7, atol=1e-7, msg=msg)
            torch.testing.assert_close(gl, gl_ref, rtol=1e-7, atol=1e-7, msg=msg)
            for a, b in zip(*runs):
                assert torch.equal(a, b), msg("two launches differ")
    finally:
        call("tce_set_cu_budget", 0)
        call("tce_pair_env_static", 1)


# (dof, nbg, T, N, pairs, uniform init times, register form allowed, budgets)
# shared covariance factor: N on both sides of the fast path's threshold (256),
# ragged last blocks for every envs-per-block count, P = 1 / 2 (no extra
# waves), 25 (12 waves), 50 / 100; K up to 64, R = 2 dof up to 16
_B0, _B2 = (0,), (0, 32)
_SHARED_CASES = [
    (3, 4, 250, 4099, 3, True, True, _B2),        # hopper
    (3, 4, 250, 256, 1, True, True, _B0),
    (3, 4, 250, 257, 100, True, True, _B0),
    (3, 4, 250, 255, 3, True, True, _B0),
    (3, 4, 250, 300, "draw", False, True, _B2),
    (3, 4, 250, 1000, 25, True, True, _B0),
    (3, 4, 250, 7, 2, True, True, _B0),
    (3, 4, 250, 1, "draw", True, True, _B0),
    (3, 4, 250, 9, 3, False, True, _B0),
    (1, 1, 100, 256, 100, True, True, _B0),
    (1, 1, 100, 4099, 2, True, True, _B0),
    (1, 1, 100, 9, 1, True, True, _B0),
    (1, 16, 129, 257, 25, True, True, _B2),
    (1, 16, 129, 1000, 3, True, True, _B0),
    (1, 16, 129, 1, 50, True, True, _B0),
    (2, 3, 65, 300, 50, True, True, _B0),
    (2, 3, 65, 255, "draw", True, True, _B0),
    (2, 3, 65, 4099, 1, True, True, _B2),
    (4, 5, 200, 256, "draw", True, True, _B0),
    (4, 5, 200, 1000, 2, True, True, _B0),
    (4, 5, 200, 7, 100, True, True, _B0),
    (4, 16, 100, 256, 3, True, True, _B2),        # K 64
    (4, 16, 100, 300, 25, True, True, _B0),
    (4, 16, 100, 9, 2, True, True, _B0),
    (5, 12, 128, 257, 2, True, True, _B0),        # K 60
    (5, 12, 128, 300, 25, True, True, _B2),
    (6, 6, 17, 1000, 3, True, True, _B2),
    (6, 6, 17, 256, 50, True, True, _B0),
    (6, 6, 17, 255, 1, True, True, _B0),
    (8, 8, 100, 256, 25, True, True, _B0),        # K 64, R 16
    (8, 8, 100, 1000, 3, True, True, _B2),
    (8, 8, 100, 300, 1, False, True, _B0),
    (8, 8, 100, 1, 3, True, True, _B0),
    (4, 6, 200, 257, 50, True, False, _B0),       # shipped shapes, LDS form
    (4, 6, 200, 4099, 3, True, False, _B2),
    (7, 9, 100, 300, 2, True, False, _B0),
    (7, 9, 100, 256, 25, True, False, _B0),
    (4, 6, 200, 257, 1, True, True, _B0),         # ... and register form
    (4, 6, 200, 1000, 25, True, True, _B2),
    (7, 9, 100, 300, 25, True, True, _B0),
    (7, 4, 130, 4099, 2, True, True, _B0),
    (7, 4, 130, 257, 50, True, True, _B0),
    (4, 9, 200, 1000, 3, True, True, _B0),
    (4, 9, 200, 256, 1, True, True, _B2),
]


@pytest.mark.parametrize("dof,nbg,T,N,pkind,uniform_t0,static,budgets",
                         _SHARED_CASES)
def test_pair_logprob_shared_factor_every_shape_vs_oracle(
        ops, dof, nbg, T, N, pkind, uniform_t0, static, budgets):
    consts = "table_tennis" if (dof, nbg) == (7, 4) else None
    _pair_case(ops, dof, nbg, T, N, pkind, True, uniform_t0, static, budgets,
               consts, seed=3 + N % 5)


_PER_ENV_CASES = [
    (3, 4, 250, 70, 25, True), (8, 8, 100, 9, 3, True), (1, 1, 100, 1, 1, True),
    (5, 12, 128, 70, 2, True), (4, 16, 100, 1, 25, True),
    (2, 3, 65, 9, 100, False), (6, 6, 17, 70, 50, False),
    (1, 16, 129, 9, "draw", True), (4, 5, 200, 70, 3, False)]


@pytest.mark.parametrize("dof,nbg,T,N,pkind,uniform_t0", _PER_ENV_CASES)
def test_pair_logprob_per_env_factor_every_shape_vs_oracle(
        ops, dof, nbg, T, N, pkind, uniform_t0):
    _pair_case(ops, dof, nbg, T, N, pkind, False, uniform_t0, seed=4 + N % 3)


_NEW_SHAPES = [(3, 4, 250), (1, 1, 100), (1, 16, 129), (2, 3, 65), (4, 5, 200),
               (4, 16, 100), (5, 12, 128), (6, 6, 17), (8, 8, 100)]


@pytest.mark.parametrize("shared,N", [(True, 300), (False, 9)])
@pytest.mark.parametrize("dof,nbg,T", _NEW_SHAPES)
def test_pair_logprob_float32_new_shapes_within_logp_rel(ops, dof, nbg, T,
                                                          shared, N):
    """Float32 buffers on the shapes no shipped document has, at the bound the
    shipped ones are held to: LOGP_REL of max |logp| from the float64 oracle on
    the same float32 inputs (fast path at 300 envs, per-env kernel at 9)."""
    dtype = F32
    cfg = cfg_of(dof, nbg, T)
    mp = make(cfg, dtype)[0]
    o64 = ProDMPOracle(dtype=F64, **cfg)
    mean, L, eps, t0, y0, v0 = inputs(cfg, N, dtype, 3, True)
    if shared:
        L = L[:1].expand(N, -1, -1).contiguous()
    times_cpu = O.get_times(t0, cfg["dt"], T)
    tg = affine(times_cpu)
    Lg = ops.expand_shared(L[0].cuda(), N) if shared else L.cuda()
    w = ops.mvn_rsample(mean.cuda(), Lg, eps.cuda())
    traj = ops.prodmp_traj(mp, tg, w, t0.cuda(), y0.cuda(), v0.cuda())
    pairs = hand_pairs(T, 25, dof)
    lp = ops.pair_log_prob(mp, traj, mean.cuda(), Lg, tg, t0.cuda(), y0.cuda(),
                           v0.cuda(), pairs.cuda())
    n = min(N, 48)
    dd = lambda x: x[:n].double()
    truth = pair_log_prob(o64, traj.cpu()[:n].double(), dd(mean), dd(L),
                          times_cpu[:n].double(), dd(t0), dd(y0), dd(v0), pairs)
    err = float((lp.cpu()[:n].double() - truth).abs().max())
    assert err <= LOGP_REL * float(truth.abs().max()), \
        (err, float(truth.abs().max()))


def test_pair_logprob_refuses_shapes_outside_the_family(ops):
    """dof * (num_basis + 1) > 64 has no pair kernel (the trajectory kernels
    take it): refused by name instead of overrunning the LDS rows."""
    cfg = cfg_of(8, 9, 100)
    mp = make(cfg, F64)[0]
    mean, L, eps, t0, y0, v0 = inputs(cfg, 4, F64, 0)
    tg = ops.times(t0.cuda(), cfg["dt"], 100)
    traj = torch.zeros(4, 100, 16, dtype=F64, device="cuda")
    for Lg in (L.cuda(), ops.expand_shared(L[0].cuda(), 4)):
        with pytest.raises(RuntimeError, match="must be <= 64"):
            ops.pair_log_prob(mp, traj, mean.cuda(), Lg, tg, t0.cuda(),
                              y0.cuda(), v0.cuda(), hand_pairs(100, 3).cuda())


# ---------------------------------------------------------------------------
# C. the backward that forms the surrogate's gradient itself
# ---------------------------------------------------------------------------
def _bwd_sur(ops, mp, traj, mean, Lb, tg, t0, y0, v0, pairs, lp_old, adv):
    """tce_pair_logprob_bwd_sur_* the way the policy epoch reaches it
    (csrc/objective.hip; flags as rl/objective.py forms them: bit 3 = all
    segments start together, bit 1 = the basis table is current)."""
    from tce_rl_amd._lib import call, ptr, sfx, stream
    N, T = tg.shape
    P, K = pairs.shape[0], mean.shape[1]
    new = lambda *s: torch.full(s, float("nan"), dtype=mean.dtype,
                                device="cuda")
    lp, gm, gL = new(N, P), new(N, K), new(K, K)
    B, flag = ops._mp_ws(mp, T, mean.device)
    work = ops._pl_work(mean, N, P, mp, 0, True)
    flags = 8 | (ops._times_flags(mp, tg, t0) & 2)
    call("tce_pair_logprob_bwd_sur_" + sfx(mean.dtype), ptr(traj), ptr(mean),
         ptr(Lb), 0, ptr(pairs), *mp.c_args(), ptr(tg), flags, ptr(t0), ptr(y0),
         ptr(v0), mp.cov_reg, ptr(lp_old), ptr(adv), ptr(lp), ptr(gm), ptr(gL),
         ptr(B), ptr(flag), ptr(work), N, T, P, mp.num_dof, stream())
    return lp, gm, gL


# (dof, nbg, T, N, pairs, register form allowed, dtype); the CPU side costs
# ~30 us per (env, pair): few pairs at 4096 envs
_SUR_CASES = [
    (3, 4, 250, 256, 25, True, F64), (3, 4, 250, 256, 25, True, F32),
    (3, 4, 250, 4096, 3, True, F32),
    (4, 6, 200, 300, "draw", True, F64), (4, 6, 200, 300, "draw", True, F32),
    (4, 6, 200, 4096, 3, True, F64), (4, 6, 200, 300, 25, False, F64),
    (7, 9, 100, 256, 6, True, F64), (7, 9, 100, 256, 6, True, F32),
    (7, 9, 100, 300, "draw", True, F32),
    (7, 4, 130, 300, 25, True, F64), (7, 4, 130, 300, 25, True, F32),
    (7, 4, 130, 4096, 6, True, F32)]


@pytest.mark.parametrize("dof,nbg,T,N,pkind,static,dtype", _SUR_CASES)
def test_surrogate_backward_vs_autograd_through_the_oracle(
        ops, dof, nbg, T, N, pkind, static, dtype):
    """d / d mean and tril(d / d L) of -mean(exp(logp - logp_old) adv) from ONE
    kernel pass (what the policy epoch runs) against autograd through the
    float64 oracle on the same inputs, and against the two-step route: forward
    kernels, the surrogate's gradient formed in torch, ordinary backward."""
    from tce_rl_amd._lib import call
    consts = "table_tennis" if (dof, nbg) == (7, 4) else None
    cfg = cfg_of(dof, nbg, T, consts)
    mp, _, mean, L, t0, y0, v0, times_cpu, traj = _pair_setup(
        cfg, T, N, dtype, True, True, seed=5)
    o64 = ProDMPOracle(dtype=F64, **cfg)
    pairs = _pairs(T, pkind, 5)
    P = pairs.shape[0]
    g = torch.Generator().manual_seed(N + P)
    adv = torch.randn(N, P, generator=g, dtype=dtype)
    noise = 0.1 * torch.randn(N, P, generator=g, dtype=F64)
    d = lambda x: x.double()
    orc = lambda dloss: oracle_logp_and_grads(
        o64, d(traj), d(mean), d(L), True, d(times_cpu), d(t0), d(y0), d(v0),
        pairs, dloss)
    # the old log-probs: the oracle's own plus noise, rounded to the dtype ONCE
    # and given to both sides (the gradient scales with the ratio)
    lp_old = (orc(lambda lp, sl: lp.sum() * 0)[0] + noise).to(dtype)
    lp_ref, gm_ref, gl_ref = orc(lambda lp, sl: -(
        (lp - lp_old[sl].double()).exp() * adv[sl].double()).sum() / (N * P))
    tg = affine(times_cpu)
    c = lambda x: x.cuda().contiguous()
    call("tce_pair_env_static", int(static))
    try:
        lp, gm, gL = _bwd_sur(ops, mp, c(traj), c(mean), c(L[0]), tg, c(t0),
                              c(y0), c(v0), c(pairs), c(lp_old), c(adv))
        # two-step route
        m2 = c(mean).requires_grad_(True)
        L2 = c(L[0]).requires_grad_(True)
        lp2 = ops.pair_log_prob(mp, c(traj), m2, ops.expand_shared(L2, N), tg,
                                c(t0), c(y0), c(v0), c(pairs))
        glp = -((lp2.detach() - c(lp_old)).exp() * c(adv)) / (N * P)
        lp2.backward(glp)
    finally:
        call("tce_pair_env_static", 1)
    gL = torch.tril(gL)
    if dtype == F64:
        tol = lambda ref: dict(rtol=1e-7, atol=1e-7)
        same = lambda ref: dict(rtol=1e-10, atol=1e-11 * float(ref.abs().max()))
        torch.testing.assert_close(lp.cpu(), lp_ref, rtol=1e-8, atol=1e-8)
    else:
        # test_objective_gpu.test_logprob_backward_with_z_matches_autograd's
        # float32 bound (rtol 2e-4, atol 2e-5), the absolute part tightened to
        # 1e-4 of the tensor's scale where that is less: the factor's gradient
        # is H^T (S - sg C^-1) M summed over N P float32 terms that cancel --
        # largest seen 5.3e-5 of scale ((7, 4), 4096 envs, one diagonal entry)
        tol = lambda ref: dict(rtol=2e-4, atol=min(
            2e-5, 1e-4 * float(ref.abs().max())))
        same = tol
        err = float((lp.cpu().double() - lp_ref).abs().max())
        assert err <= LOGP_REL * float(lp_ref.abs().max()), err
    torch.testing.assert_close(gm.cpu().double(), gm_ref, **tol(gm_ref))
    torch.testing.assert_close(gL.cpu().double(), gl_ref, **tol(gl_ref))
    torch.testing.assert_close(gm, m2.grad, **same(gm_ref))
    torch.testing.assert_close(gL, torch.tril(L2.grad), **same(gl_ref))
    torch.testing.assert_close(lp, lp2.detach(), **same(lp_ref))


def test_surrogate_backward_refuses_what_it_cannot_take(ops):
    """Per-env factors, fewer than 256 envs or init times not known to be equal
    have no inline-surrogate form: refused, never a silent other path."""
    cfg = cfg_of(3, 4, 250)
    mp, _, mean, L, t0, y0, v0, times_cpu, traj = _pair_setup(
        cfg, 250, 255, F64, True, True)
    pairs = hand_pairs(250, 3)
    z = torch.zeros(255, 3, dtype=F64, device="cuda")
    c = lambda x: x.cuda().contiguous()
    with pytest.raises(RuntimeError, match="needs the shared-factor fast path"):
        _bwd_sur(ops, mp, c(traj), c(mean), c(L[0]), affine(times_cpu), c(t0),
                 c(y0), c(v0), c(pairs), z, z)
