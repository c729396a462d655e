"""CPU: the engine flag --window_record_passes (ic3net_amd.main) — known to the parser, an int, off by default — and what the
Trainer makes of it before any launch (Trainer._record_passes, the gate in front of the passes' record of begin_episode): no for
hid 256, one pass, more than four, a zero-padded twin, no --window_launch, a window that would not play, a policy that does not know
the argument, and no memory room; yes where all of it holds.  The ops-level query answers for hid 64 / 128 and passes 2..4 only."""
import inspect
import itertools
from types import SimpleNamespace

from ic3net_amd import _lib, bptt, main, ops
from ic3net_amd.trainer import Trainer


def parse(argv):
    argv = ['main.py'] + argv
    return main.build_parser(argv).parse_args(argv[1:])


def test_the_parser_knows_the_flag_and_it_is_off_by_default():
    a = parse([])
    assert a.window_record_passes == 0 and isinstance(a.window_record_passes, int)
    assert a.window_launch is False and a.window_launch_collection == 0 and a.multipass_window_collection == 0   # no default moved
    a = parse(['--window_record_passes', '1', '--env_name', 'predator_prey'])
    assert a.window_record_passes == 1 and a.window_launch is False                                      # independent switches
    assert ('window_record_passes', int, 0) in main._ENGINE_FLAGS


def test_the_ops_query_answers_for_hid_64_128_and_2_to_4_passes_only(monkeypatch):
    for f in (ops.policy_step_window_supported, ops.policy_step_window):
        assert inspect.signature(f).parameters['record_passes'].default in (False, None)
    monkeypatch.setattr(ops, 'policy_step_supported', lambda env, H: True)                              # (the handle says yes)
    planes = dict(ps_l_wp3=object())
    for H, passes in itertools.product((32, 64, 128, 200, 256), range(0, 7)):
        assert bool(ops.policy_step_window_supported(None, planes, H, passes=passes, record_passes=True)) == \
            (H in (64, 128) and 2 <= passes <= 4), (H, passes)
        assert not ops.policy_step_window_supported(None, dict(), H, passes=passes, record_passes=True)  # no split planes
    monkeypatch.setattr(ops, 'policy_step_supported', lambda env, H: False)
    assert not ops.policy_step_window_supported(None, planes, 64, passes=2, record_passes=True)
    assert _lib.PolicyWindowRecord.WINDOW_PASSES_RECORD == 9
    assert (_lib.PolicyWindow.WINDOW, _lib.PolicyWindow.WINDOW_PASSES, _lib.PolicyWindow.WINDOW_WIDE, _lib.PolicyWindow.WINDOW_WIDE_PASSES) == \
        (3, 5, 6, 8)


class _Policy(object):
    def __init__(self, passes=2, hid=64):
        self.comm_passes, self.hid_size, self.asked = passes, hid, []

    def window_supported(self, env, wide=False, wide_passes=False, record_passes=False):
        self.asked.append(record_passes)
        return self.hid_size in (64, 128)


class _KnowsNothingOfIt(_Policy):
    def window_supported(self, env, wide=False, wide_passes=False):
        return True


def _gate(monkeypatch, net=None, knet=None, room=1 << 40, window_ok=True, **flags):
    """Trainer._record_passes for a window of T = 8 steps of R = 36 rows, every question it does not ask itself answered as given."""
    import torch
    net = net or _Policy()
    tr = Trainer.__new__(Trainer)
    tr.args = SimpleNamespace(**dict(dict(window_launch=True, window_record_passes=1), **flags))
    tr.env = SimpleNamespace(env=object())
    tr.policy_net = net
    tr._window_launch_ok = lambda check_every=0: window_ok
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(bptt, 'device_room', lambda dev: room)
    return Trainer._record_passes(tr, net if knet is None else knet, 8, 36)


def test_the_gate_in_front_of_the_record(monkeypatch):
    assert _gate(monkeypatch) is True
    assert _gate(monkeypatch, net=_Policy(passes=4, hid=128)) is True
    assert not _gate(monkeypatch, window_record_passes=0)
    assert not _gate(monkeypatch, window_launch=False)                                                   # no --window_launch
    assert not _gate(monkeypatch, net=_Policy(hid=256))                                                  # hid 256
    assert not _gate(monkeypatch, net=_Policy(passes=1)) and not _gate(monkeypatch, net=_Policy(passes=5))
    assert not _gate(monkeypatch, knet=_Policy())                                                        # a zero-padded twin runs the launches
    assert not _gate(monkeypatch, window_ok=False)                                                       # the window would not play
    assert not _gate(monkeypatch, net=_KnowsNothingOfIt())                                               # called as before: no record
    # the rule of _record_gates: T * R * (P * 6H + (P - 1) * 2H) * 4 bytes within half the room
    need = 8 * 36 * (2 * 6 * 64 + 2 * 64) * 4
    assert _gate(monkeypatch, room=2 * need) is True and not _gate(monkeypatch, room=2 * need - 2) and not _gate(monkeypatch, room=0)
    asked = _Policy()
    _gate(monkeypatch, net=asked)
    assert asked.asked == [True]
