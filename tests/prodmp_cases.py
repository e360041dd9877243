"""Inputs shared by the ProDMP GPU tests (tests/test_prodmp_gpu.py: the shipped
shapes; tests/test_prodmp_shapes_gpu.py: the whole family the kernels accept).
Every helper takes the MP constants as a config dict (the keyword arguments of
``ProDMP`` / ``ProDMPOracle``)."""
import torch

from oracle import tce_oracle as O
from oracle.prodmp_oracle import ProDMPOracle


def make(cfg, dtype):
    """-> (the product's ProDMP on the GPU, the CPU oracle) of one config."""
    from tce_rl_amd.mp import ProDMP
    return ProDMP(dtype=dtype, device="cuda", **cfg), \
        ProDMPOracle(dtype=dtype, **cfg)


def affine(times_cpu):
    """The oracle's own time grid on the GPU, tagged like ops.times() output:
    isolates the kernels under test from the last-bit differences of the
    float32 linspace weights (machine dependent on the CPU side)."""
    t = times_cpu.cuda()
    t._tce_affine = True
    return t


def inputs(cfg, N, dtype, seed=0, uniform_t0=True):
    """-> mean [N, K], L [N, K, K], eps [N, K], t0 [N], y0, v0 [N, dof]."""
    dof, K = cfg["num_dof"], cfg["num_dof"] * (cfg["num_basis"] + 1)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    mean = 0.5 * rn(N, K)
    L = O.vector_to_cholesky(
        torch.cat([rn(N, K), 0.05 * rn(N, K * (K - 1) // 2)], -1), K, 1e-4,
        False)
    eps = rn(N, K)
    y0 = torch.rand(N, dof, generator=g, dtype=dtype) * 2 - 1
    v0 = 0.1 * rn(N, dof)
    t0 = torch.zeros(N, dtype=dtype) if uniform_t0 else \
        torch.rand(N, generator=g, dtype=dtype) * 0.2
    return mean, L, eps, t0, y0, v0
