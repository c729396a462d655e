"""The case table of tests/test_full_flags_update_gpu.py: every policy family under the COMPLETE fast setting — all the one-launch
switches of ic3net_amd.main._ENGINE_FLAGS on at once — and, per row, the path the update must take, as counter values after one
train_batch.  Plain data: nothing here imports torch, bench or the library (tests/test_full_flags_cases_cpu.py reads it without a
GPU).

The expectations are written from the flag documentation in ic3net_amd/main.py (_ENGINE_FLAGS), not from a run:
  window_launch                every recorded window of max_steps lock-steps is ONE launch where the policy supports it
  window_launch_collection     ... collection-mode windows (auto_reset) too
  window_launch_wide           ... at hid 256 too: the one-pass LSTM policy, the non-recurrent module, IC, IRIC-tanh — NOT IRIC's LSTM cell
  passes_in_launch_wide        comm_passes 2..4 at hid 256: the passes inside the launch, and with the two above the window in one launch
  backward_walk                IRIC-tanh: the window's backward in one launch (rnn_backward_walks)
  backward_walk_lstm           LSTM policies without communication whose rollout kept a gate record: IRIC-LSTM at hid 64 / 128,
                               recurrent CommNet under comm_mask_zero at 64 / 128 / 256 (lstm_backward_walks); policies that
                               communicate and comm_passes > 1 never walk
  window_record_passes         comm_passes 2..4 at hid 64 / 128: the window launch records the passes, the update reads the record
                               (multipass_recorded_windows); hid 256 and zero-padded twins keep the re-evaluation
  multipass_window_collection  comm_passes > 1 in collection mode runs the window backward (multipass_window_backwards)
  commnet_window_backward / multipass_window_backward   (default 1) the window-wide backward of the non-recurrent module / of
                               comm_passes > 1
Shapes: the smallest that still cut windows and tiles — max_steps 6 with detach_gap 4 (a cut inside every window), two windows per
update, 16 envs; collection rows: 32 envs of a 2-agent 3 x 3 Predator-Prey grid, whose episodes end and restart inside windows."""

T_STEPS, WINDOWS, SEED, ENV_OFFSET = 6, 2, 5, 0
E_LOCKSTEP, E_COLLECTION = 16, 32

# every path switch of ic3net_amd.main._ENGINE_FLAGS, at its fast setting
FULL_FLAGS = dict(window_launch=True, window_launch_collection=1, window_launch_wide=1, passes_in_launch_wide=1, backward_walk=1,
                  backward_walk_lstm=1, window_record_passes=1, multipass_window_collection=1,
                  commnet_window_backward=1, multipass_window_backward=1)     # (the last two: their default)
# ... and the entries of _ENGINE_FLAGS that choose no path of the update
NOT_PATH_SWITCHES = ('nenvs', 'device', 'hip_graph', 'tune_gemm', 'dist_backend')

HYPER = dict(gamma=0.95, entr=0.01, value_coeff=0.01, advantages_per_action=False)

# workloads beside bench.WORKLOADS (registered with bench.WORKLOADS.setdefault by tests/full_flags_util.py)
EXTRA_WORKLOADS = {
    'full_flags_tj_easy': ("traffic_junction", dict(nagents=5, dim=6, vision=1, max_steps=T_STEPS, hid_size=128, ic3net=True,
                                                    recurrent=True, detach_gap=4, difficulty='easy', add_rate_min=0.3,
                                                    add_rate_max=0.3)),
}

_PP = dict(nagents=3, dim=5, vision=1, max_steps=T_STEPS, detach_gap=4)
_PP_TINY = dict(nagents=2, dim=3, vision=1, max_steps=T_STEPS, detach_gap=4)
_ZERO_COMM = dict(ic3net=False, commnet=True, comm_mask_zero=True)

COUNTERS = ('window_launches', 'per_step', 'lstm_backward_walks', 'rnn_backward_walks', 'multipass_window_backwards',
            'multipass_recorded_windows', 'commnet_window_backwards')


def _expect(**kw):
    """Counter values after the update; what is not named stays 0.  'W' = one per window, 'WT' = one per recorded step."""
    unknown = set(kw) - set(COUNTERS)
    assert not unknown, unknown
    return {k: {'W': WINDOWS, 'WT': WINDOWS * T_STEPS, 0: 0}[kw.get(k, 0)] for k in COUNTERS}


CASES = []


def _row(row, workload, over, hids, expect, because, collection=(), because_collection=(), tj=False, **more):
    """One table row: a lock-step case per hidden size and a collection case for every size in `collection`.  `expect` /
    `because`: dicts by hidden size, or one value for all of them."""
    for hid in hids:
        for mode in ['lock-step'] + (['collection'] if hid in collection else []):
            coll = mode == 'collection'
            shape = dict(over if tj and not coll else dict(_PP_TINY if coll else _PP, **over), hid_size=hid)
            shape.update(max_steps=T_STEPS, detach_gap=4)
            wl = workload if not (tj and coll) else more['collection_workload']
            why = tuple(because[hid] if isinstance(because, dict) else because) + (tuple(because_collection) if coll else ())
            CASES.append(dict(name="%s-h%d-%s" % (row, hid, mode), row=row, workload=wl, overrides=shape, hid=hid, mode=mode,
                              envs=E_COLLECTION if coll else E_LOCKSTEP,
                              expect=dict(expect[hid] if hid in expect else expect), because=why,
                              normalize_rewards=bool(more.get('normalize_rewards')) and not coll, refused=False))


_COLL = ('window_launch_collection',)
# IC3Net, one pass: the window in one launch; it communicates, so nothing walks
_row('ic3', 'pp_easy', {}, [64], _expect(window_launches='W'), ('window_launch',), collection=[64], because_collection=_COLL)
_row('ic3-tj', 'full_flags_tj_easy', dict(), [128], _expect(window_launches='W'), ('window_launch',), tj=True, normalize_rewards=True)
_row('ic3-wide', 'pp_easy', {}, [256], _expect(window_launches='W'), ('window_launch', 'window_launch_wide'), collection=[256],
     because_collection=_COLL)
# comm_passes 2..4 at hid 64 / 128: the window records its passes, the update reads them
_row('ic3-p2', 'pp_easy', dict(comm_passes=2), [64],
     _expect(window_launches='W', multipass_window_backwards='W', multipass_recorded_windows='W'),
     ('window_launch', 'window_record_passes', 'multipass_window_backward'), collection=[64],
     because_collection=_COLL + ('multipass_window_collection',))
_row('ic3-p3s', 'full_flags_tj_easy', dict(comm_passes=3, share_weights=True), [128],
     _expect(window_launches='W', multipass_window_backwards='W', multipass_recorded_windows='W'),
     ('window_launch', 'window_record_passes', 'multipass_window_backward'), tj=True)
# ... at hid 256: the window in one launch (passes inside), but no record of the passes — the update re-evaluates them
_row('ic3-p2-wide', 'pp_easy', dict(comm_passes=2), [256], _expect(window_launches='W', multipass_window_backwards='W'),
     ('window_launch', 'window_launch_wide', 'passes_in_launch_wide', 'multipass_window_backward'))
# recurrent CommNet whose communication block sees zeros: the window in one launch and its backward walked in one launch
_row('zero-comm', 'pp_hard', _ZERO_COMM, [128, 256], _expect(window_launches='W', lstm_backward_walks='W'),
     {128: ('window_launch', 'backward_walk_lstm'), 256: ('window_launch', 'window_launch_wide', 'backward_walk_lstm')},
     collection=[128], because_collection=_COLL)
# IRIC with the LSTM cell: hid 64 as above; hid 256 keeps one launch per step (window_launch_wide leaves it alone) and — no gate
# record at that width — the per-step backward
_row('iric-lstm', 'pp_hard_iric', {}, [64, 256],
     {64: _expect(window_launches='W', lstm_backward_walks='W'), 256: _expect(per_step='WT')},
     {64: ('window_launch', 'backward_walk_lstm'), 256: ('window_launch_wide', 'backward_walk_lstm')},
     collection=[64], because_collection=_COLL)
# IRIC with the tanh recurrence: window launch (hid 256: wide) and the walk of --backward_walk
_row('iric-tanh', 'pp_hard_iric_tanh', {}, [128, 256], _expect(window_launches='W', rnn_backward_walks='W'),
     {128: ('window_launch', 'backward_walk'), 256: ('window_launch', 'window_launch_wide', 'backward_walk')},
     collection=[128], because_collection=_COLL)
# IC (models.MLP): window launch; no state crosses a step, nothing to walk
_row('ic-mlp', 'pp_hard_ic', {}, [64, 256], _expect(window_launches='W'),
     {64: ('window_launch',), 256: ('window_launch', 'window_launch_wide')}, collection=[64], because_collection=_COLL)
# the non-recurrent CommNet module, two passes, gated (IC3Net without recurrence): window launch + the window-wide backward
_row('mlp2', 'full_flags_tj_easy', dict(recurrent=False, comm_passes=2), [64, 256],
     _expect(window_launches='W', commnet_window_backwards='W'),
     {64: ('window_launch', 'commnet_window_backward'), 256: ('window_launch', 'window_launch_wide', 'commnet_window_backward')},
     collection=[64], because_collection=_COLL, tj=True, collection_workload='pp_easy')
# hid 48 runs as its zero-padded twin at 64: one launch per step, the window backward on the twin, the passes re-evaluated
_row('twin', 'pp_easy', dict(comm_passes=2), [48], _expect(per_step='WT', multipass_window_backwards='W'),
     ('window_launch', 'window_record_passes', 'multipass_window_backward'))

BY_NAME = {c['name']: c for c in CASES}
