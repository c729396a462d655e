"""GPU: Trainer.train_batch on the non-recurrent CommNet module with the window backward (bptt._backward_window_commnet, one
ic3_commnet_backward call per recorded episode) against the same update through the per-step loop (bptt._backward_episode_commnet):
same seed, hence the same rollout and the same losses; the path counter says which backward ran; every parameter's gradient within
its bar against the loop's (tests/commnet_window_bars.py: 4 x the measured worst |window - loop| / max |loop| per parameter)."""
import numpy as np
import pytest
import torch

import commnet_window_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = {
    # IC3Net's non-recurrent module on TJ-easy: hard-attention gates, cars entering and leaving (dead agents), two passes
    'gpu_trainer_tj_easy': ("traffic_junction", dict(nagents=5, dim=6, vision=1, max_steps=10, hid_size=64, ic3net=True, recurrent=False,
                                                     comm_passes=2, difficulty='easy', add_rate_min=0.3, add_rate_max=0.3), 24),
    # CommNet on a small Predator-Prey grid: hid 128, one F and one C shared by three passes
    'gpu_trainer_pp': ("predator_prey", dict(nagents=3, dim=5, vision=1, max_steps=8, hid_size=128, commnet=True, recurrent=False,
                                             comm_passes=3, share_weights=True, mode='mixed'), 22),
    # a window the library is made to run in chunks of three steps (a short last chunk)
    'gpu_trainer_pp_chunks': ("predator_prey", dict(nagents=3, dim=5, vision=1, max_steps=8, hid_size=64, commnet=True, recurrent=False,
                                                    comm_passes=2, mode='mixed'), 22),
}


def _update(name, window):
    import bench
    env_name, flags, E = SHAPES[name]
    bench.WORKLOADS.setdefault(name, (env_name, flags))
    tr, a = bench.build_trainer(name, E, 3, 70, 0)
    T = flags['max_steps']
    a.__dict__.update(gamma=0.95, normalize_rewards=True, entr=0.01, value_coeff=0.01, advantages_per_action=False, batch_size=E * T,
                      commnet_window_backward=window)
    if name.endswith('_chunks'):
        a.commnet_window_chunk_steps = 3
    assert tr._native_update()
    stat = tr.train_batch(0)
    torch.cuda.synchronize()
    net = tr._kernel_net()
    assert getattr(tr.policy_net, 'commnet_steps', 0) >= T, "the one-launch rollout did not run"
    grads = {k: p.grad.double().cpu().numpy() for k, p in tr.policy_net.named_parameters() if p.grad is not None}
    return stat, grads, getattr(net, 'commnet_window_backwards', 0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_train_batch_window_against_loop(name):
    s1, g1, n1 = _update(name, True)
    s0, g0, n0 = _update(name, False)
    assert n1 >= 1 and n0 == 0, "which backward ran: window %d, loop %d" % (n1, n0)
    for k in ("action_loss", "value_loss", "entropy", "num_steps"):
        assert s1[k] == s0[k], k
    assert set(g1) == set(g0) and g1
    errs = {}
    for k in g0:
        scale = max(float(np.abs(g0[k]).max()), 1e-12)
        assert np.isfinite(g1[k]).all() and scale > 1e-9, k
        errs[k] = float(np.abs(g1[k] - g0[k]).max() / scale)
    ref.check(name, errs)
