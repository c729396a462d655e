"""CPU: the engine flag --window_launch_wide (ic3net_amd.main) — known to the parser, an int, off by default, beside the switches it
acts with; what the Trainer makes of it before any launch: a hid-256 policy is asked for its window with `wide` set only with the flag;
and the defaults of the ops-level queries, which keep today's answers at hid 256."""
import inspect
from types import SimpleNamespace

from ic3net_amd import _lib, main, ops
from ic3net_amd.trainer import Trainer


def parse(argv):
    argv = ['main.py'] + argv
    return main.build_parser(argv).parse_args(argv[1:])


def test_the_parser_knows_the_flag_and_it_is_off_by_default():
    a = parse([])
    assert a.window_launch_wide == 0 and isinstance(a.window_launch_wide, int)
    assert a.window_launch is False and a.window_launch_collection == 0             # no default moved
    a = parse(['--window_launch', '--window_launch_wide', '1', '--env_name', 'predator_prey'])
    assert a.window_launch is True and a.window_launch_wide == 1 and a.window_launch_collection == 0
    a = parse(['--window_launch', '--window_launch_wide', '1', '--window_launch_collection', '1', '--env_name', 'predator_prey'])
    assert a.window_launch_wide == 1 and a.window_launch_collection == 1            # independent switches
    assert ('window_launch_wide', int, 0) in main._ENGINE_FLAGS


class _Hid256(object):
    """A policy that answers as a hid-256 module does: its window only with `wide`."""

    def __init__(self):
        self.asked = []

    def commnet_window_supported(self, env, wide=False):
        self.asked.append(wide)
        return bool(wide)


def _ok(**flags):
    """Trainer._window_launch_ok on a stand-in of the non-recurrent family in front of a lock-step window, every other question
    answered yes."""
    tr = Trainer.__new__(Trainer)
    tr.args = SimpleNamespace(window_launch=True, recurrent=False, rnn_type='MLP', hid_size=256, store_states=False, **flags)
    tr._rec, tr.env = SimpleNamespace(recurrent=False), SimpleNamespace(env=SimpleNamespace(auto_max_steps=0))
    tr.policy_net = _Hid256()
    tr._auto_reset = lambda: False
    tr._dense_obs = lambda: False
    tr._commnet_expected = lambda raw: True
    return Trainer._window_launch_ok(tr), tr.policy_net.asked


def test_a_hid_256_window_is_asked_for_only_with_the_flag():
    assert _ok() == (False, [False])                                               # as before: the policy answers no
    assert _ok(window_launch_wide=0) == (False, [False])
    assert _ok(window_launch_wide=1) == (True, [True])


def test_the_ops_queries_keep_their_answers_at_hid_256():
    assert inspect.signature(ops.policy_step_window_supported).parameters['wide'].default is False
    assert inspect.signature(ops.commnet_step_window_supported).parameters['wide'].default is False
    assert inspect.signature(ops.policy_step_window).parameters['wide'].default is False
    assert inspect.signature(ops.commnet_step_window).parameters['wide'].default is False
    planes = dict(ps_l_wp3=object(), wp3=object())
    # (answered from the hidden size, in front of anything that looks at the handle)
    assert ops.policy_step_window_supported(None, planes, 256) is False
    assert ops.commnet_step_window_supported(None, planes, 256) is False
    for hid in (64, 128):                                                           # the wide tags mean hid 256 and nothing else
        assert ops.policy_step_window_supported(None, planes, hid, wide=True) is False
        assert ops.commnet_step_window_supported(None, planes, hid, wide=True) is False
    assert not ops.policy_step_window_supported(None, dict(), 256, wide=True)       # no split planes
    assert not ops.commnet_step_window_supported(None, dict(), 256, wide=True)
    assert (_lib.PolicyWindow.WINDOW, _lib.PolicyWindow.WINDOW_PASSES, _lib.CommnetWindow.WINDOW) == (3, 5, 4)
    assert (_lib.PolicyWindow.WINDOW_WIDE, _lib.CommnetWindow.WINDOW_WIDE) == (6, 7)
