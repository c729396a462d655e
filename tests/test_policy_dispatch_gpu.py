"""GPU: which path every policy family takes through the Trainer — the one-launch step, the zero-padded twin, the baselines'
kernel stand-in or the launch chain — per hidden size and per switch.  The expected table was recorded by running these
same rows on the commit before the policy modules' one-copy pass (comm.py / models.py) and is not edited by hand: the
launch predicates (mega_ok, mega_supported, commnet_step_ok, rnn_step_ok, _fused_ok, _commnet_ok) keep their truth tables.

Shapes: Predator-Prey, 5 agents, dim 10, vision 1, 5 envs, one episode of 3 steps per row."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, E = 3, 5
SHAPE = dict(nagents=5, dim=10, vision=1, max_steps=T)

# family -> (bench workload it starts from, flags)
FAMILIES = {
    'ic3_p1': ('pp_hard', dict()),                                                      # IC3Net LSTM, one pass
    'ic3_p2': ('pp_hard', dict(comm_passes=2)),                                         # IC3Net LSTM, two passes
    'commnet_lstm': ('pp_hard', dict(ic3net=False, commnet=True)),                      # CommNet LSTM, hard_attn off
    'mlp2': ('pp_hard', dict(ic3net=False, commnet=True, recurrent=False, comm_passes=2)),   # non-recurrent module, 2 passes
    'mlp2_share': ('pp_hard', dict(ic3net=False, commnet=True, recurrent=False, comm_passes=2, share_weights=True)),
    'ic_mlp': ('pp_hard_ic', dict()),                                                   # models.MLP
    'iric_tanh': ('pp_hard_iric_tanh', dict()),                                         # models.RNN, tanh recurrence
    'iric_lstm': ('pp_hard_iric', dict()),                                              # models.RNN, LSTM cell
}

# row -> (family, hid_size, switches).  What each group exercises:
#   <family>-64    the kernels' own size: _mega_wanted / ops.commnet_forward_supported hold, kernel_module() is the policy (or,
#                  for a baseline, the Trainer's fallback: the baseline itself), every env / step-tensor clause holds
#   <family>-16    ops.padded_hidden(16) = 64: _twin() (pad_hidden, fused_policy, mega_policy, <= 4 heads, LSTM when
#                  recurrent, fp32 on the device); a baseline's stand-in runs as ITS twin; rnn_step_supported's
#                  `padded_hidden is None` clause turns the tanh recurrence down
#   <family>-260   no kernel size and no twin: `hid_size in POLICY_STEP_SIZES` / commnet_forward_supported fail -> the
#                  launch chain (_fused_ok without _mega_wanted for one pass; _multi_pass_ok fails for two -> generic forward)
#   -no_mega       args.mega_policy off: _mega_wanted, _commnet_ok's mega_policy clause, the twin's and the stand-in's
#   -no_fused      args.fused_policy off: the first-layer clause of _fused_ok / _commnet_ok / mega_supported, and the twin's
#   -no_pad        args.pad_hidden off: only the twin asks (no difference at 64; at 16 no kernel size is left)
#   -grad          args.rollout_grad: Trainer._launch_path_base and the grad-mode clause of every step predicate
ROWS = {}
for _f in FAMILIES:
    for _h in (64, 16, 260):
        ROWS['%s-%d' % (_f, _h)] = (_f, _h, dict())
for _f in ('ic3_p1', 'mlp2'):
    for _h in (64, 16):
        for _sw in ('mega_policy', 'fused_policy', 'pad_hidden'):
            ROWS['%s-%d-no_%s' % (_f, _h, _sw.split('_')[0])] = (_f, _h, {_sw: False})
for _f in FAMILIES:
    ROWS['%s-64-grad' % _f] = (_f, 64, dict(rollout_grad=True))
assert len(ROWS) <= 48

COLUMNS = ('mega_steps', 'commnet_steps', 'mega_forwards', 'commnet_forwards', 'kernel_module_is_self', 'mega_supported',
           'mega_supported_no_grad')

# Recorded on the parent commit (see the module docstring); columns as COLUMNS.  mega_supported: None = the policy has no such
# method; asked in the default grad mode, as Trainer.begin_episode asks it, and once more under torch.no_grad().
EXPECTED = {
    'ic3_p1-64': (3, 0, 0, 0, True, True, True),
    'ic3_p1-16': (3, 0, 0, 0, False, True, True),
    'ic3_p1-260': (0, 0, 0, 0, True, False, False),
    'ic3_p2-64': (3, 0, 0, 0, True, True, True),
    'ic3_p2-16': (3, 0, 0, 0, False, True, True),
    'ic3_p2-260': (0, 0, 0, 0, True, False, False),
    'commnet_lstm-64': (3, 0, 0, 0, True, True, True),
    'commnet_lstm-16': (3, 0, 0, 0, False, True, True),
    'commnet_lstm-260': (0, 0, 0, 0, True, False, False),
    'mlp2-64': (0, 3, 0, 0, True, False, False),
    'mlp2-16': (0, 3, 0, 0, False, False, False),
    'mlp2-260': (0, 0, 0, 0, True, False, False),
    'mlp2_share-64': (0, 3, 0, 0, True, False, False),
    'mlp2_share-16': (0, 3, 0, 0, False, False, False),
    'mlp2_share-260': (0, 0, 0, 0, True, False, False),
    'ic_mlp-64': (0, 3, 0, 0, True, None, None),
    'ic_mlp-16': (0, 3, 0, 0, True, None, None),
    'ic_mlp-260': (0, 0, 0, 0, True, None, None),
    'iric_tanh-64': (0, 3, 0, 0, True, False, False),
    'iric_tanh-16': (0, 0, 0, 0, True, False, False),
    'iric_tanh-260': (0, 0, 0, 0, True, False, False),
    'iric_lstm-64': (3, 0, 0, 0, True, False, True),
    'iric_lstm-16': (3, 0, 0, 0, True, False, True),
    'iric_lstm-260': (0, 0, 0, 0, True, False, False),
    'ic3_p1-64-no_mega': (0, 0, 0, 0, True, False, False),
    'ic3_p1-64-no_fused': (0, 0, 0, 0, True, False, False),
    'ic3_p1-64-no_pad': (3, 0, 0, 0, True, True, True),
    'ic3_p1-16-no_mega': (0, 0, 0, 0, True, False, False),
    'ic3_p1-16-no_fused': (0, 0, 0, 0, True, False, False),
    'ic3_p1-16-no_pad': (0, 0, 0, 0, True, False, False),
    'mlp2-64-no_mega': (0, 0, 0, 0, True, False, False),
    'mlp2-64-no_fused': (0, 0, 0, 0, True, False, False),
    'mlp2-64-no_pad': (0, 3, 0, 0, True, False, False),
    'mlp2-16-no_mega': (0, 0, 0, 0, True, False, False),
    'mlp2-16-no_fused': (0, 0, 0, 0, True, False, False),
    'mlp2-16-no_pad': (0, 0, 0, 0, True, False, False),
    'ic3_p1-64-grad': (0, 0, 0, 0, True, True, True),
    'ic3_p2-64-grad': (0, 0, 0, 0, True, True, True),
    'commnet_lstm-64-grad': (0, 0, 0, 0, True, True, True),
    'mlp2-64-grad': (0, 0, 0, 0, True, False, False),
    'mlp2_share-64-grad': (0, 0, 0, 0, True, False, False),
    'ic_mlp-64-grad': (0, 0, 0, 0, True, None, None),
    'iric_tanh-64-grad': (0, 0, 0, 0, True, False, False),
    'iric_lstm-64-grad': (0, 0, 0, 0, True, False, True),
}


def measure(row):
    import bench
    family, hid, switches = ROWS[row]
    workload, flags = FAMILIES[family]
    tr, a = bench.build_trainer(workload, E, 3, 0, 0, **dict(SHAPE, hid_size=hid, **dict(flags, **switches)))
    net, raw = tr.policy_net, tr.env.env
    episode, _ = tr.get_episode(0)
    assert len(episode) == T
    sup = getattr(net, 'mega_supported', None)
    with torch.no_grad():
        sup_ng = None if sup is None else bool(sup(raw))
    return tuple(int(getattr(net, k, 0)) for k in COLUMNS[:4]) + (
        tr._kernel_net() is net, None if sup is None else bool(sup(raw)), sup_ng)


@pytest.mark.parametrize("row", list(ROWS))
def test_policy_dispatch_table(row):
    got = measure(row)
    print(row, dict(zip(COLUMNS, got)))
    assert got == EXPECTED[row], dict(zip(COLUMNS, zip(got, EXPECTED[row])))
