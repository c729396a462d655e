"""GPU: the update with EVERY one-launch switch on at once (tests/full_flags_cases.py: window_launch, window_launch_collection,
window_launch_wide, passes_in_launch_wide, backward_walk, backward_walk_lstm, window_record_passes, multipass_window_collection)
against a float64 replay that shares no kernel with it (tests/full_flags_util.py: plain torch autograd through the policy modules'
generic forward, on the flagged batch's own actions).  Per (row, hid, mode):

  path      the counters after the update equal the row's expectation, written from the flag documentation of ic3net_amd/main.py; the
            native update ran; no window was refused
  rollout   the replay saw the same episode: reward, episode_mask, episode_mini_mask, every misc['alive_mask'] and misc['live'],
            num_steps and num_episodes bit-equal — the env stepping and restarts inside the launch and ic3_episode_finalize behind it
  forward   batch.value and the log-probability of every taken action against float64
  update    action_loss, value_loss, entropy (relative) and every parameter's gradient (max |g - g64| / max(max |g64|, 1e-6))
            against float64; the set of parameters with a gradient equals float64's

Bars: nothing is fixed in advance.  The same run replays the tape in torch fp32 as well; its error against float64, per tensor and
per loss, is e_ref, and the bar is max(8 x e_ref, 4e-6) for gradients and forward quantities, max(8 x e_ref, 2e-6) for losses: 8 =
twice the worst ratio the project has recorded between its fixed-order fp32 chains and torch's blocked sums (heads.1.weight,
1.08e-5 against 2.8e-6, profiles/r06/grad_errors.txt); the floors are tests/test_trainer_gpu.py's GRAD_TOL floors.  No bar may
exceed 1e-4.  IC3_FULL_FLAGS_ERRORS_OUT=<file> appends every figure; one run is kept in profiles/r29/full_flags_errors.txt.

The sensitivity control scales ONE weight entry of the flagged trainer by 1 + 1e-3 and asserts that the comparison then fails."""
import pytest

from full_flags_cases import CASES, WINDOWS

pytestmark = pytest.mark.gpu


def _run(case, before=None):
    import torch
    from full_flags_util import compare, flagged_update, replay, rollout_differences
    flagged = flagged_update(case, before)
    assert flagged['native'], "the native update did not run"
    tape = torch.stack(list(flagged['batch'].action)).clone()
    truth, stick = replay(case, tape, torch.float64), replay(case, tape, torch.float32)
    rollout = rollout_differences(flagged, truth) + ['fp32 replay: ' + k for k in rollout_differences(flagged, stick)]
    return flagged, truth, stick, rollout, compare(case, flagged, truth, stick)


def _over_the_bar(rows):
    from full_flags_util import CAP
    bad = []
    for k, err, e_ref, bar in rows:                                # (each figure in front of the assertions)
        print("full-flags %-34s flagged %.3e   e_ref %.3e   bar %.3e" % (k, err, e_ref, bar))
        if not (bar <= CAP and err <= bar):                        # (a missing figure is nan: over the bar)
            bad.append((k, err, e_ref, bar))
    return bad


@pytest.mark.parametrize("case", CASES, ids=[c['name'] for c in CASES])
def test_full_flags_update_matches_the_float64_replay(case):
    flagged, truth, stick, rollout, rows = _run(case)
    # path
    assert flagged['windows'] == WINDOWS
    assert flagged['counters'] == case['expect'], (flagged['counters'], case['expect'])
    assert flagged['refused'] == case['refused']
    # rollout
    assert not rollout, "the replay did not see the flagged episode: %r" % rollout
    # forward and update: nothing left out, the same parameters carry a gradient
    assert set(flagged['grads']) == set(truth['grads']) == set(stick['grads'])
    names = {r[0] for r in rows}
    assert {'grad:' + k for k in truth['grads']} <= names and {'loss:action_loss', 'loss:value_loss', 'loss:entropy',
                                                                'forward:value', 'forward:logp_taken.0'} <= names
    bad = _over_the_bar(rows)
    assert not bad, "%s: (quantity, flagged error, e_ref, bar) %r" % (case['name'], bad)


@pytest.mark.parametrize("which,row", [("C_modules.0.weight", False), ("f_module.weight_hh", False), ("f_module.weight_hh", True)],
                         ids=["C_modules.0.weight", "f_module.weight_hh", "f_module.weight_hh-row"])
def test_the_bars_see_one_weight_entry_scaled_by_a_thousandth(which, row):
    """ONE entry of the communication weight / the LSTM's recurrent weight of the FLAGGED trainer times 1 + 1e-3: the comparison
    against the replay of the unscaled weights must fail for some tensor.  `row`: one whole row of the weight instead, the shape of
    error a stale weight plane makes.

    Which entry: the one the update depends on most, read off the float64 replay of the unscaled update — the largest
    |dL/dw x w|, i.e. the entry whose scaling by a given factor moves the loss most to first order (the row: the largest sum of it).
    The control therefore shows that the bars see a relative 1e-3 in the most influential entry, NOT in an arbitrary one: most of the
    4096 entries of a 64 x 64 weight carry almost nothing, and the entry of largest |w| alone moved no figure past its bar (nearest
    grad:f_module.weight_ih, 1.99e-6 against 4.18e-6).  Figures: profiles/r29/full_flags_errors.txt, the rows tagged /scaled."""
    import torch
    from full_flags_cases import BY_NAME
    case = BY_NAME['ic3-h64-lock-step']
    _, plain, _, rollout, _ = _run(dict(case, name=case['name'] + '/control-unscaled'))
    assert not rollout
    weight = (plain['grads'][which].double() * plain['params'][which].double()).abs()
    pick = int(weight.sum(1).argmax()) if row else int(weight.argmax())
    print("full-flags control: %s %s %d" % (which, "row" if row else "entry", pick))

    def before(tr, a):
        w = dict(tr.policy_net.named_parameters())[which]
        with torch.no_grad():
            if row:
                w[pick] *= 1.0 + 1e-3
            else:
                w.view(-1)[pick] *= 1.0 + 1e-3
    tag = '/scaled:' + which + ('-row' if row else '')
    flagged, truth, stick, rollout, rows = _run(dict(case, name=case['name'] + tag), before)
    assert not rollout, "the replay did not see the flagged episode: %r" % rollout
    assert _over_the_bar(rows), "no tensor left its bar: the bars do not see an error of this size"
