"""tce_rl_amd/streams.py: side streams are PROBED -- a HIP stream is bound to a
hardware queue when it is created, streams that share a queue wait for each
other's kernels, and which queue a new stream lands on depends on how many
streams the process created before.  A side stream is handed out only if a
kernel on it demonstrably runs while one on the default stream (and on every
side stream handed out before) is still running."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_spin_kernel_lasts_what_it_is_asked_to():
    from tce_rl_amd._lib import call, stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call("tce_spin_us", 50.0, stream())              # warm
    torch.cuda.synchronize()
    e0.record()
    call("tce_spin_us", 2000.0, stream())
    e1.record()
    torch.cuda.synchronize()
    # at least what was asked for (the upper end is the launch's business: the
    # probe only compares two spins with each other)
    assert 1.9 <= e0.elapsed_time(e1) <= 200.0
    with pytest.raises(RuntimeError, match="spin_us"):
        call("tce_spin_us", 0.0, stream())


def test_side_streams_run_beside_the_default_stream_and_each_other():
    from tce_rl_amd import streams
    from tce_rl_amd._lib import call
    names = ("policy", "objective", "graph")
    got = dict(zip(names, (streams.get(n) for n in names)))
    assert streams.get("policy") is got["policy"]    # process-wide
    # the HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES
    # hardware queues (4 unless the host sets fewer); the default stream holds
    # one, so that many side streams less one can have a queue to themselves.
    # Those the probe must have found (whichever test asked for them first);
    # for the rest it must have said that there is none
    queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    found = {n: ok for n, _, ok in streams.PROBE_LOG if n in names}
    own = [got[n] for n in names if found[n]]
    assert len(own) == min(len(names), queues - 1)
    assert len({s.cuda_stream for s in own}) == len(own)
    main = torch.cuda.default_stream()
    every = [main] + own
    for i, a in enumerate(every):
        for b in every[i + 1:]:
            assert streams._beside(b, a) and streams._beside(a, b)
    for n in names:
        if not found[n]:
            assert not all(streams._beside(got[n], o) for o in every)
    # the probe itself tells shared queues apart: a stream does not run beside
    # itself
    assert not streams._beside(own[0], own[0])
    # all of them busy at once: the wall time is one spin, not one per stream
    torch.cuda.synchronize()
    t = time.perf_counter()
    for s in every:
        call("tce_spin_us", 3000.0, s.cuda_stream)
    torch.cuda.synchronize()
    assert time.perf_counter() - t < 0.006
