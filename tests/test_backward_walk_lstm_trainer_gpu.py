"""GPU: args.backward_walk_lstm — the update of an LSTM policy WITHOUT communication walks a recorded window's backward through time in
ONE launch (bptt._backward_window_native -> ops.bptt_backward(walk=True) -> ic3_bptt_backward on an ic3_bptt_walk descriptor) — against
the per-step launches of the same tree: two train_batch updates from one seed with the flag 0 and with the flag 1, as
tests/test_backward_walk_trainer_gpu.py does for the tanh recurrence.  PP, 3 agents, dim 5, 16 envs, max_steps 6, detach_gap 4:
  IRIC with the LSTM cell (pp_hard_iric: models.RNN on its stand-in) at hid 64 / 128, lock-step and collection mode (auto_reset, two
  windows per update);  a recurrent CommNet policy under comm_mask_zero at hid 256, lock-step.
Every parameter and the RMSprop state must be bit-identical after both updates, and lstm_backward_walks — counted on the policy the
trainer holds, for IRIC the owning models.RNN — equals the number of windows with the flag and 0 without.  Policies the walk does not
cover (pp_hard: it communicates; pp_hard_iric_tanh: --backward_walk's) run unchanged with the flag set: the counter stays 0 and the
parameters are flag 0's bit for bit.

ON BOTH SIDES the encoder's window finish is its ordered form (see tests/test_backward_walk_trainer_gpu.py: the plain finish adds with
float atomics, and two flag-0 trainings do not repeat themselves through it); the flag does not touch it.  What the flag does change is
compared bit for bit on the library call itself in tests/test_lstm_walk_gpu.py."""
import pytest
import torch

from test_window_launch_trainer_gpu import _equal

pytestmark = pytest.mark.gpu

T_STEPS, E_ENVS, WINDOWS, UPDATES = 6, 16, 2, 2
_PP = dict(nagents=3, dim=5, vision=1, max_steps=T_STEPS, detach_gap=4)
# a recurrent CommNet policy (no hard attention) whose communication block sees zeros (comm.py:40-41)
_MASK_ZERO = dict(ic3net=False, commnet=True, comm_mask_zero=True)


def _train(workload, hid, collection, walk, **over):
    """UPDATES train_batch calls; returns the parameters, the optimizer's state and the counters."""
    import bench
    tr, a = bench.build_trainer(workload, E_ENVS, 5, 0, 0, **dict(_PP, hid_size=hid, **over))
    a.__dict__.update(gamma=0.95, normalize_rewards=False, entr=0.01, value_coeff=0.01, advantages_per_action=False,
                      batch_size=WINDOWS * E_ENVS * a.max_steps)
    a.auto_reset = bool(collection)
    a.backward_walk_lstm = int(walk)
    raw = tr.env.env                                             # (see the module's docstring: the finish that repeats itself)
    ordered = raw.encode_backward_window_finish_ordered
    finishes, windows = [0], [0]

    def finish(H, want_bias=True):
        finishes[0] += 1
        return ordered(H, want_bias=want_bias)
    raw.encode_backward_window_finish = finish
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
                walks=getattr(net, 'lstm_backward_walks', 0), tanh_walks=getattr(net, 'rnn_backward_walks', 0), windows=windows[0],
                finishes=finishes[0], owner=type(net).__name__)


def _compare(tag, off, on):
    assert any(s for s in on['rmsprop'].values())
    for k in on['params']:                                       # (each figure in front of the assertions)
        print("backward-walk-lstm %s %s: max |on - off| %.3e" % (tag, k, (on['params'][k] - off['params'][k]).abs().max().item()))
    _equal(on['params'], off['params'], "parameters")
    _equal(on['rmsprop'], off['rmsprop'], "RMSprop state")


@pytest.mark.parametrize("collection", [False, True], ids=["lock-step", "collection"])
@pytest.mark.parametrize("hid", [64, 128])
def test_iric_lstm_update_equals_the_per_step_update(hid, collection):
    off = _train('pp_hard_iric', hid, collection, 0)
    on = _train('pp_hard_iric', hid, collection, 1)
    assert on['owner'] == 'RNN'                                  # (the counter sits on the owning models.RNN, not its stand-in)
    assert off['windows'] == on['windows'] == UPDATES * WINDOWS
    assert off['walks'] == 0 and on['walks'] == on['windows'], "the walk did not run every window's backward"
    assert off['finishes'] == on['finishes'] == UPDATES * WINDOWS, "the window backward did not go through the encoder's window form"
    _compare("iric hid %d %s" % (hid, "collection" if collection else "lock-step"), off, on)


def test_recurrent_commnet_under_comm_mask_zero_at_hid_256():
    off = _train('pp_hard', 256, False, 0, **_MASK_ZERO)
    on = _train('pp_hard', 256, False, 1, **_MASK_ZERO)
    assert on['owner'] == 'CommNetMLP'
    assert off['windows'] == on['windows'] == UPDATES * WINDOWS
    assert off['walks'] == 0 and on['walks'] == on['windows'], "the walk did not run every window's backward"
    assert off['finishes'] == on['finishes'] == UPDATES * WINDOWS
    _compare("commnet comm_mask_zero hid 256", off, on)


@pytest.mark.parametrize("workload", ['pp_hard', 'pp_hard_iric_tanh'])
def test_policies_the_walk_does_not_cover_run_unchanged(workload):
    off = _train(workload, 64, False, 0)
    on = _train(workload, 64, False, 1)
    assert on['walks'] == off['walks'] == 0 and on['tanh_walks'] == 0 and on['windows'] == UPDATES * WINDOWS
    _compare(workload, off, on)
