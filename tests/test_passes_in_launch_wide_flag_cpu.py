"""CPU: the engine flag --passes_in_launch_wide (ic3net_amd.main) — known to the parser, an int, off by default, beside the switches it
acts with; what the Trainer makes of it before any launch: a policy is asked for its window with `wide_passes` only with the flag (a
policy or a stand-in that knows `wide` alone is called as before); and the ops-level queries, which keep today's answers with the
keyword off at every argument combination."""
import inspect
import itertools
from types import SimpleNamespace

from ic3net_amd import _lib, main, ops
from ic3net_amd.trainer import Trainer


def parse(argv):
    argv = ['main.py'] + argv
    return main.build_parser(argv).parse_args(argv[1:])


def test_the_parser_knows_the_flag_and_it_is_off_by_default():
    a = parse([])
    assert a.passes_in_launch_wide == 0 and isinstance(a.passes_in_launch_wide, int)
    assert a.window_launch is False and a.window_launch_collection == 0 and a.window_launch_wide == 0   # no default moved
    a = parse(['--passes_in_launch_wide', '1', '--env_name', 'predator_prey'])
    assert a.passes_in_launch_wide == 1 and a.window_launch is False and a.window_launch_wide == 0       # independent switches
    a = parse(['--window_launch', '--window_launch_wide', '1', '--passes_in_launch_wide', '1', '--window_launch_collection', '1',
               '--env_name', 'predator_prey'])
    assert (a.window_launch, a.window_launch_wide, a.passes_in_launch_wide, a.window_launch_collection) == (True, 1, 1, 1)
    assert ('passes_in_launch_wide', int, 0) in main._ENGINE_FLAGS and ('window_launch_wide', int, 0) in main._ENGINE_FLAGS


def _before(fc, H, passes, wide):
    """policy_step_passes_supported / policy_step_window_supported as they answered before the keyword existed (in front of anything
    that looks at the handle: the handle is asked last, and only where everything else said yes)."""
    p_ok = 2 <= passes <= 4 and H in (64, 128) and fc.get('ps_l_wp3') is not None
    if passes != 1 and not p_ok:
        return p_ok, False
    if wide:
        return p_ok, None if (H == 256 and passes == 1 and fc.get('ps_l_wp3') is not None) else False
    return p_ok, None if (H in (64, 128) and fc.get('ps_l_wp3') is not None) else False


def test_the_ops_queries_keep_their_answers_with_the_keyword_off(monkeypatch):
    for f in (ops.policy_step_passes_supported, ops.policy_step_window_supported, ops.policy_step_window):
        assert inspect.signature(f).parameters['wide_passes'].default is False
    asked = []
    monkeypatch.setattr(ops, 'policy_step_supported', lambda env, H: asked.append(H) or True)   # (the handle says yes)
    for planes, H, passes, wide in itertools.product((dict(ps_l_wp3=object()), dict()), (32, 64, 128, 200, 256), range(0, 7),
                                                     (False, True)):
        p_ok, w_ok = _before(planes, H, passes, wide)
        assert bool(ops.policy_step_passes_supported(planes, H, passes)) == p_ok, (H, passes)
        del asked[:]
        got = ops.policy_step_window_supported(None, planes, H, passes=passes, wide=wide)
        assert bool(got) == (w_ok is None), (H, passes, wide)
        assert bool(asked) == (w_ok is None), "the handle is asked exactly where it was"
    planes = dict(ps_l_wp3=object())
    # hid 256 with passes >= 2 stays False without the keyword — under either existing tag
    for passes in (2, 3, 4):
        assert ops.policy_step_passes_supported(planes, 256, passes) is False
        assert ops.policy_step_window_supported(None, planes, 256, passes=passes) is False
        assert ops.policy_step_window_supported(None, planes, 256, passes=passes, wide=True) is False
    # and with it: hid 256 and 2..4 passes, nothing else
    for H, passes in itertools.product((64, 128, 256), range(1, 7)):
        assert bool(ops.policy_step_passes_supported(planes, H, passes, wide_passes=True)) == (2 <= passes <= 4)
        assert bool(ops.policy_step_window_supported(None, planes, H, passes=passes, wide_passes=True)) == \
            (passes <= 4 if H != 256 else 2 <= passes <= 4)
    assert not ops.policy_step_passes_supported(dict(), 256, 2, wide_passes=True)       # no split planes
    assert not ops.policy_step_window_supported(None, dict(), 256, passes=2, wide_passes=True)
    assert _lib.PolicyWindow.WINDOW_WIDE_PASSES == 8
    assert (_lib.PolicyWindow.WINDOW, _lib.PolicyWindow.WINDOW_PASSES, _lib.PolicyWindow.WINDOW_WIDE) == (3, 5, 6)


class _KnowsWide(object):
    """A policy (or a test stand-in) from before the keyword: its window_supported takes `wide` alone."""
    comm_passes = 1

    def __init__(self):
        self.asked = []

    def window_supported(self, env, wide=False):
        self.asked.append(dict(wide=wide))
        return True


class _KnowsBoth(_KnowsWide):
    comm_passes = 2

    def window_supported(self, env, wide=False, wide_passes=False):
        self.asked.append(dict(wide=wide, wide_passes=wide_passes))
        return bool(wide and wide_passes)


def _ok(net, **flags):
    """Trainer._window_launch_ok on a stand-in of the LSTM family in front of a lock-step window, every other question answered yes."""
    import torch
    tr = Trainer.__new__(Trainer)
    tr.args = SimpleNamespace(window_launch=True, recurrent=True, rnn_type='LSTM', hid_size=256, store_states=False, **flags)
    one = net.comm_passes == 1
    tr._rec = SimpleNamespace(recurrent=True, gates=object() if one else None, xh=torch.empty(1, 1, 256) if one else None,
                              hs=torch.empty(1, 1, 256))
    tr.env = SimpleNamespace(env=SimpleNamespace(auto_max_steps=0))
    tr.policy_net = net
    tr._auto_reset = lambda: False
    tr._dense_obs = lambda: False
    tr._mega_expected = lambda raw: True
    tr._rec_inplace = lambda: True
    return Trainer._window_launch_ok(tr), net.asked


def test_the_trainer_passes_the_keyword_only_under_the_flag():
    wide = dict(window_launch_wide=1)
    # two passes: asked with wide_passes exactly when the flag is set
    assert _ok(_KnowsBoth(), **wide) == (False, [dict(wide=True, wide_passes=False)])
    assert _ok(_KnowsBoth(), passes_in_launch_wide=0, **wide) == (False, [dict(wide=True, wide_passes=False)])
    assert _ok(_KnowsBoth(), passes_in_launch_wide=1, **wide) == (True, [dict(wide=True, wide_passes=True)])
    assert _ok(_KnowsBoth(), passes_in_launch_wide=1) == (False, [dict(wide=False, wide_passes=True)])     # (no --window_launch_wide)
    # a policy that knows `wide` alone is called as today without the flag (no TypeError), one pass and two
    assert _ok(_KnowsWide(), **wide) == (True, [dict(wide=True)])
    two = _KnowsWide()
    two.comm_passes = 2
    assert _ok(two, **wide) == (True, [dict(wide=True)])
