"""Generate ``multi_episode.npz``: what the REFERENCE's own samplers return for
rollouts of several episodes per environment.

``mprl.rl.sampler.TemporalCorrelatedSampler`` / ``BlackBoxSampler`` are
subclassed with ``get_env`` overridden, so that ``run()`` itself executes on
the CPU against the scripted numpy vec env and the closed-form stub policy /
critic of ``tests/fake_vec_env.py`` (float64; nothing random but the pair
draw).  Stored per case and run: every key of the result dict, the step count,
``pred_pairs``, the final ``obs_rms.mean / var / count`` and one draw from
torch's global generator taken after ``run()``.  tests/test_multi_episode_gpu.py
drives this repository's samplers with the same objects and compares.

Runs ONLY where the reference tree is present (like make_golden.py, whose
import stubs it uses); the ``.npz`` is committed, the reference never travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_multi_episode.py [--out DIR]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_golden import import_reference                    # noqa: E402
from tests import fake_vec_env as F                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    import_reference()
    from mprl.rl.sampler import BlackBoxSampler, TemporalCorrelatedSampler

    def scripted(base, case):
        fn = F.scripted_env_fn(case)

        class Scripted(base):
            def get_env(self, env_type="training"):
                n = {"training": self.num_env_train,
                     "testing": self.num_env_test, "debugging": 1}[env_type]
                return fn(env_id=self.env_id, num_env=n, seed=self.seed,
                          render=False, mp_args=self.mp_args)
        return Scripted

    arrays = {}
    for case, c in F.MULTI_EPISODE_CASES.items():
        base = TemporalCorrelatedSampler if c["kind"] == "tc" \
            else BlackBoxSampler
        sampler = scripted(base, case)(**F.sampler_kwargs(case, "cpu"))
        for i, rec in enumerate(F.run_case(case, sampler)):
            for k, v in rec.items():
                v = v.detach().cpu().numpy() if torch.is_tensor(v) \
                    else np.asarray(v)
                arrays["%s__run%d__%s" % (case, i, k)] = v
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "multi_episode.npz")
    # (np.savez stamps no time into the archive: the same arrays give the same
    # bytes)
    np.savez_compressed(path, **arrays)
    print("wrote", path, len(arrays), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
