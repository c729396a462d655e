"""GPU: args.backward_walk — the update of IRIC with the tanh recurrence (models.RNN, rnn_type 'MLP') walks a recorded window's
backward through time in ONE launch (bptt._backward_window_rnn -> ops.rnn_backward(walk=True) -> ic3_rnn_backward_wide on an
ic3_rnn_bptt_walk descriptor) — against the per-step launches of the same tree: two train_batch updates from one seed with the flag 0
and with the flag 1.  PP, 3 agents, dim 5, 16 envs, max_steps 6, detach_gap 4 (R = 48: one tile, so the bias partials correspond row
by row); hid 64 / 128 / 256; lock-step, and collection mode (auto_reset) with two windows per update; each also with the rollout's
window launch on both sides (window_launch, at 256 window_launch_wide too).  Every parameter and the RMSprop state must be
bit-identical after both updates, and rnn_backward_walks equals the number of windows.  A policy the walk does not cover (IC, IRIC
with the LSTM cell) runs unchanged with the flag set and its counter stays 0.

ON BOTH SIDES the encoder's window finish is its ordered form (Env.encode_backward_window_finish_ordered in place of
encode_backward_window_finish, which _backward_window_rnn calls).  The plain finish adds affine1.weight's gradient with float atomics,
and two flag-0 trainings from one seed do not repeat themselves through it: measured on the MI355X, flag 0 against flag 0 after two
updates differs by up to 8.2e-08 in affine1.weight (and, from the second update on, in every parameter) — as much as flag 1 against
flag 0 (up to 6.7e-08; profiles/r26/backward_walk_trainer.txt).  Bit equality of a pair of runs can only be asked where a run
equals itself; the ordered finish reads the same stage-1 sums, sums them in a fixed order, and is not touched by the flag.  What the
flag does change — the launch that produces dz, dh, the bias partials and a2_grad — is compared bit for bit on the library call itself
in tests/test_tanh_walk_gpu.py."""
import pytest
import torch

from test_window_launch_trainer_gpu import _equal

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS, WINDOWS, UPDATES = 6, 16, 2, 2
_PP = dict(nagents=3, dim=5, vision=1, max_steps=T_STEPS, detach_gap=4)


def _build(workload, hid, collection, window_launch, walk):
    import bench
    tr, a = bench.build_trainer(workload, E_ENVS, 5, 0, 0, **dict(_PP, hid_size=hid))
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=WINDOWS * E_ENVS * a.max_steps)
    a.auto_reset = bool(collection)
    a.window_launch = bool(window_launch)
    a.window_launch_wide = int(window_launch and hid == 256)
    a.window_launch_collection = int(window_launch and collection)
    a.backward_walk = int(walk)
    raw = tr.env.env                                             # (see the module's docstring: the finish that repeats itself)
    ordered = raw.encode_backward_window_finish_ordered
    tr.ordered_finishes = [0]

    def finish(H, want_bias=True):
        tr.ordered_finishes[0] += 1
        return ordered(H, want_bias=want_bias)
    raw.encode_backward_window_finish = finish
    return tr, a


def _train(workload, hid, collection, window_launch, walk):
    """UPDATES train_batch calls; returns the parameters, the optimizer's state and the counters."""
    tr, a = _build(workload, hid, collection, window_launch, walk)
    windows = [0]
    inner = tr.compute_grad_native

    def spy(batch, records):
        windows[0] += len(records)
        return inner(batch, records)
    tr.compute_grad_native = spy
    for u in range(UPDATES):
        tr.train_batch(u)
    torch.cuda.synchronize()
    net = tr.policy_net
    state = tr.optimizer.state_dict()['state']
    return dict(params={k: p.detach().clone() for k, p in net.named_parameters()},
                rmsprop={i: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in state.items()},
                walks=getattr(net, 'rnn_backward_walks', 0), windows=windows[0], window_launches=getattr(net, 'window_launches', 0),
                finishes=tr.ordered_finishes[0])


@pytest.mark.parametrize("window_launch", [False, True], ids=["step-rollout", "window-launch"])
@pytest.mark.parametrize("collection", [False, True], ids=["lock-step", "collection"])
@pytest.mark.parametrize("hid", [64, 128, 256])
def test_backward_walk_update_equals_the_per_step_update(hid, collection, window_launch):
    off = _train('pp_hard_iric_tanh', hid, collection, window_launch, 0)
    on = _train('pp_hard_iric_tanh', hid, collection, window_launch, 1)
    assert off['windows'] == on['windows'] == UPDATES * WINDOWS
    assert off['walks'] == 0 and on['walks'] == on['windows'], "the walk did not run every window's backward"
    assert off['finishes'] == on['finishes'] == UPDATES * WINDOWS, "the window backward did not go through the encoder's window form"
    if window_launch:
        assert off['window_launches'] == on['window_launches'] == UPDATES * WINDOWS
    assert any(s for s in on['rmsprop'].values())
    for k in on['params']:                                       # (each figure in front of the assertions)
        d = (on['params'][k] - off['params'][k]).abs().max().item()
        print("backward-walk hid %d %s %s %s: max |on - off| %.3e" % (hid, "collection" if collection else "lock-step",
                                                                      "window-launch" if window_launch else "step-rollout", k, d))
    _equal(on['params'], off['params'], "parameters")
    _equal(on['rmsprop'], off['rmsprop'], "RMSprop state")


@pytest.mark.parametrize("workload", ['pp_hard_ic', 'pp_hard_iric'])
def test_policies_the_walk_does_not_cover_run_unchanged(workload):
    off = _train(workload, 64, False, False, 0)
    on = _train(workload, 64, False, False, 1)
    assert on['walks'] == off['walks'] == 0 and on['windows'] == UPDATES * WINDOWS
    assert all(bool(torch.isfinite(p).all()) for p in on['params'].values())
